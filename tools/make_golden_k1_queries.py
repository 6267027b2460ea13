#!/usr/bin/env python
"""Generate tests/golden/conv133_k1_queries.json: what the three K1 host queries (e2e_conv133_fwd_ws_bytes,
e2e_conv133_dgrad_ws_bytes, e2e_conv133_num_partials) answer over a fixed sweep of shapes.

    python tools/make_golden_k1_queries.py

Needs the built library and no GPU (the queries are host arithmetic); E2E_CONV_* must be unset.  The committed table was recorded
at commit f1449f4, the last one whose csrc/conv133.hip answered the queries from pick_tile / plan_fwd_ksplit / plan_dgrad_ksplit;
tests/test_host_cpu.py::test_k1_queries_equal_the_parent holds the K1 plan that replaced them to it.  Regenerating at a later commit
records that commit's answers: do so only when a change of the plan is meant.

Rows run over itertools.product(B, Cin, Cout, dims, strides) in that order; num_partials takes the row's output dims and in-plane
stride (it has no B, Cin or Cout)."""
import itertools
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SWEEP = {
    "B": [1, 2],
    "Cin": [1, 4, 16, 17, 40, 320, 896],
    "Cout": [8, 32, 33, 320],
    "dims": [[2, 4, 4], [5, 7, 5], [8, 8, 8], [4, 16, 16], [3, 12, 40], [3, 9, 20], [4, 17, 20], [6, 32, 64], [3, 40, 64], [16, 128, 128]],
    "strides": [list(s) for s in itertools.product((1, 2), repeat=3)],
}


def rows(sweep=SWEEP):
    return itertools.product(sweep["B"], sweep["Cin"], sweep["Cout"], sweep["dims"], sweep["strides"])


def query(L, row):
    b, cin, cout, (di, hi, wi), (sd, sh, sw) = row
    do, ho, wo = (di - 1) // sd + 1, (hi - 1) // sh + 1, (wi - 1) // sw + 1
    return (int(L.conv133_fwd_ws_bytes(b, cin, cout, di, hi, wi, sd, sh, sw)),
            int(L.conv133_dgrad_ws_bytes(b, cin, cout, di, hi, wi, sd, sh, sw)),
            int(L.conv133_num_partials(do, ho, wo, sh, sw)))


def main():
    assert not [k for k in os.environ if k.startswith("E2E_CONV_")], "record with E2E_CONV_* unset"
    import torch  # noqa: F401  (the HIP runtime of PyTorch-ROCm must be loaded before the library)
    from e2enet_medical_amd._lib import lib
    L = lib()
    got = [query(L, r) for r in rows()]
    fwd, dgrad, parts = (list(c) for c in zip(*got))
    assert len(fwd) == 4480 and sum(v > 0 for v in fwd) >= 200 and sum(v > 0 for v in dgrad) >= 200
    commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    out = dict(SWEEP, commit=commit, fwd_ws_bytes=fwd, dgrad_ws_bytes=dgrad, num_partials=parts)
    path = os.path.join(ROOT, "tests", "golden", "conv133_k1_queries.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    print("%s: %d rows, %d / %d split forward / data gradient, %d bytes" %
          (path, len(fwd), sum(v > 0 for v in fwd), sum(v > 0 for v in dgrad), os.path.getsize(path)))


if __name__ == "__main__":
    main()
