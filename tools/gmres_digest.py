"""SHA-256 of (X, info, inner, status) of every GMRES case of the test tables: a bitwise before / after check for changes to
csrc/gmres.hip that must not change any result (tools, not product).   python tools/gmres_digest.py [--out FILE]

Cases: every case of tests/gmres_cases.py through run_case under the default schedule (method 0: the dense shared mode, the CSR
mode, the dense mode of DENSE_TAILS, band_n* at all BOUNDARY_SIZES, so every register instantiation of the post kernel and the
streamed one), then every CSR case of that table (the *_csr cases and band_n*) and every case of tests/gmres_wide_cases.py
under the wide step (method 1).
MAUS_LIB names an older build of the library, for the "before" digests."""
import argparse
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from adaptive_matrix_solver_amd import _cabi  # noqa: E402
if os.environ.get("MAUS_LIB"):                               # an older build of the library, for the "before" digests
    _cabi.LIB_PATH = os.environ["MAUS_LIB"]
import gmres_cases as gc  # noqa: E402
import gmres_wide_cases as gw  # noqa: E402


def is_csr(case):
    return bool(case["build"]()["csr"])


def digest(got):
    X, info, inner, status = got
    h = hashlib.sha256()
    h.update(np.ascontiguousarray(X, dtype=np.complex128).tobytes())
    for v in (info, inner, status):
        h.update(np.ascontiguousarray(v, dtype=np.int64).tobytes())
    return h.hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    a = ap.parse_args()
    plan = [(_cabi.GMRES_DEFAULT, c) for c in gc.CASES]
    plan += [(_cabi.GMRES_WIDE, c) for c in gc.CASES if is_csr(c)] + [(_cabi.GMRES_WIDE, c) for c in gw.CASES]
    ctx = _cabi.Context(0)
    print(f"# library {os.path.relpath(_cabi.load_library()._name, ROOT)}", flush=True)
    lines = []
    for method, case in plan:
        ctx.gmres_set_method(method)
        got = gc.run_case(ctx, case)
        line = (f"method {method} {case['name']:<28} info {int(got[1][0]):>2} inner {int(got[2][0]):>4} "
                f"status {int(np.abs(got[3]).sum())} sha256 {digest(got)}")
        print(line, flush=True)
        lines.append(line)
    ctx.close()
    print(f"# {len(lines)} cases, sha256 of all lines {hashlib.sha256(chr(10).join(lines).encode()).hexdigest()}", flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
