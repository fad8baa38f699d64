// Prints the plan maus_mt_plan makes for a dense regulariser run (tests/test_pop_draw_host.py compares it with its own
// statement of the arithmetic).  Built with the host compiler together with csrc/mtplan.cpp; no HIP.
//   mt_plan_dump n pos g wpc lead s_override ord_0 ... ord_{g-1}
// Output, whitespace separated: S E ngen dj dj2 nlevels | per level: off count J src_off multi | len(hs) hs...
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../adaptive_matrix_solver_amd/csrc/mtplan.h"

int main(int argc, char** argv) {
    if (argc < 8) return 2;
    const int n = atoi(argv[1]), g = atoi(argv[3]), s_override = atoi(argv[6]);
    if (argc != 7 + g) return 2;
    maus_mt_desc d;
    std::memset(&d, 0, sizeof d);
    d.pos = atoi(argv[2]);
    d.words_per_candidate = strtoull(argv[4], nullptr, 10);
    d.lead_words = strtoull(argv[5], nullptr, 10);
    std::vector<int32_t> ords(g);
    for (int k = 0; k < g; ++k) ords[k] = atoi(argv[7 + k]);
    d.ordinals = ords.data();
    MausMtPlan pl;
    const char* err = nullptr;
    if (maus_mt_plan(&d, n, 0, g, s_override, &pl, &err)) { std::fprintf(stderr, "%s\n", err ? err : "failed"); return 1; }
    std::printf("%d %llu %d %llu %llu %zu\n", pl.S, (unsigned long long)pl.E, pl.ngen, (unsigned long long)pl.dj,
                (unsigned long long)pl.dj2, pl.levels.size());
    for (const auto& L : pl.levels)
        std::printf("%zu %d %llu %d %d\n", L.off, L.count, (unsigned long long)L.J, L.src_off, L.multi ? 1 : 0);
    std::printf("%zu", pl.hs.size());
    for (int v : pl.hs) std::printf(" %d", v);
    std::printf("\n");
    return 0;
}
