#!/usr/bin/env python3
"""Digest of the conv weight gradient on every path: for each conv row of WGRAD_WS_CASES (tests/test_gpu_ops.py), under the
default environment, E2E_WG_BF3=0 (the fp32-MFMA kernels) and E2E_WG_H2=0 (bf16 three-piece operands), one line with the
dispatch note and the SHA-256 of dw.  The weight gradient is deterministic, so two trees that compute the same thing print the
same lines: run it on both and diff.

    python tools/wgrad_digest.py [--root TREE]      # TREE: the checkout whose package, library and table are used (default: this one)

The knobs are read once per process, so each environment runs in a child process."""
import argparse
import hashlib
import os
import subprocess
import sys

ENVS = [{}, {"E2E_WG_BF3": "0"}, {"E2E_WG_H2": "0"}]


def digest_rows(root, tag):
    sys.path.insert(0, root)
    import torch
    from tests import test_gpu_ops as T
    from e2enet_medical_amd.engine import ConvOp
    from e2enet_medical_amd._lib import lib
    from tests.helpers import seeded_input
    L = lib()
    for case in T.WGRAD_WS_CASES:
        family, B, cin, cout, dims, sk = case[:6]
        if family != "conv":
            continue
        src = T._make_act((B, cin) + dims, True, 90)
        e = T._eng_stub({"blk.conv.weight": torch.zeros(cout, cin, 1, 3, 3), "blk.conv.bias": torch.zeros(cout),
                         "blk.instnorm.weight": torch.ones(cout), "blk.instnorm.bias": torch.zeros(cout)})
        op = ConvOp(e, "blk", [src], cout, sk)
        op.set_input_range(float(T._act_value(src).abs().max()))
        dy = seeded_input((B, cout) + op.out_dims, seed=91).cuda()
        word = T._absmax_word(dy)
        dw = torch.full((cout, cin, 1, 3, 3), float("nan"), device="cuda")
        L.conv133_wgrad(op.chans.data_ptr(), dy.data_ptr(), dw.data_ptr(), e.wgrad_ws.data_ptr(), B, cin, cout, *dims, *sk,
                        word.data_ptr(), op.x_absmax_ptr(), 0)
        torch.cuda.synchronize()
        note = (L.last_kernel() or b"").decode()
        sha = hashlib.sha256(dw.cpu().numpy().tobytes()).hexdigest()
        print("%s B=%d %d->%d %s stride %s | %s | %s" % (tag, B, cin, cout, dims, sk, note, sha), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--child", help=argparse.SUPPRESS)
    args = ap.parse_args()
    root = os.path.abspath(args.root)
    if args.child is not None:
        digest_rows(root, args.child)
        return 0
    for env in ENVS:
        tag = " ".join("%s=%s" % kv for kv in env.items()) or "default"
        child_env = {k: v for k, v in os.environ.items() if k not in ("E2E_WG_BF3", "E2E_WG_H2")}
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--root", root, "--child", tag], env=dict(child_env, **env), cwd=root)
        if r.returncode != 0:
            return r.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
