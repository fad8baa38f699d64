// Host-side plan of the device MT19937 regeneration (MAUS_PERT_MT19937): which generator start states a sub-batch
// needs and how they are reached from the one NumPy state by binary lifting.  Pure host arithmetic -- no HIP -- so that
// it builds under the CPU sanitizers together with mt19937.cpp (`make asan`).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>
#include "../../include/maus_hip.h"

struct MausMtPlan {
    int S = 1;                 // sub-streams per rand(N,N) draw (one workgroup each)
    uint64_t E = 0;            // elements per sub-stream
    int ngen = 0;              // generators = 2 draws x g candidates x S sub-streams
    uint64_t dj = 0, dj2 = 0;  // jump strides in blocks of 624 words: per draw, per sub-stream
    // staging image for the device: extra[ngen] (real block regenerations after the jumps) | rpos[ngen] (position in the
    // block) | the selection list of every lifting level
    std::vector<int> hs;
    // states[hs[off + i]] <- x^(mult_i * J) applied to states[hs[off + i] - src_off]   (src_off = 0: in place).
    // multi: hs[off + count + i] = mult_i in 1..15 (one hexadecimal digit of the draw index per level); else mult_i = 1
    struct Level { size_t off; int count; uint64_t J; int src_off; bool multi; };
    std::vector<Level> levels;
};

// Candidates [first, first+g) of a run described by d (n x n matrices).  s_override > 0 forces the sub-stream count.
// Returns 0, or -1 with *err set.
int maus_mt_plan(const maus_mt_desc* d, int n, int first, int g, int s_override, MausMtPlan* out, const char** err);
// The same for draws of `L` elements (maus_mt_plan is L = n*n with the dense regulariser's rule): at most s_cap sub-streams per
// draw, each at least min_sub elements long and a multiple of e_align.
int maus_mt_plan_len(const maus_mt_desc* d, uint64_t L, int first, int g, int s_override, int s_cap, uint64_t min_sub,
                     uint64_t e_align, MausMtPlan* out, const char** err);
// Candidate vectors (maus_pop_draw): `count` pairs of rand(len) draws at d->ordinals[0..count), the rule of a vector draw.
#define MAUS_POP_DRAW_MIN_SUB (256 * 312)
#define MAUS_POP_DRAW_CHUNK (16 * 312)          // elements per partial sum of the squared norm (mtdev.hip)
int maus_pop_draw_plan_desc(const maus_mt_desc* d, int len, int count, int substreams, MausMtPlan* out, const char** err);
