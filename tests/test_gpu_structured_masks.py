"""The DSFF conv paths on kernel maps with structure, against fp64.

Every other test draws its kernel map entry by entry (`rand < density`), and at the channel counts of the tests such a map
practically never holds what a trained one does (kernel_death empties whole filters, growth refills elsewhere): an output channel
without a live kernel, an input channel nobody reads, an aligned block of 8 dead input planes, a liveness word that is zero, one
row that carries many times the mean work.  Four places depend on the SHAPE of the map and not only on its density:
  * the flush interval of the load-balanced kernel's two-level summation (conv133_sparse.hip: derived from the MEAN live count);
  * first-writer semantics of the data gradient: a concat input plane without a live kernel is zero-filled by the op that writes
    the gradient buffer first and left alone by one that writes later, on every kernel family;
  * an output plane without a live kernel is its bias, a constant: InstanceNorm variance 0, rstd = 1 / sqrt(eps) ~ 316;
  * the plan's geometry at its limits: a fully live 32-plane group (kmax = 256) and waves whose every liveness word is 0.
The maps come from helpers.structured_kmask, the truth is an fp64 torch-CPU evaluation of the same graph, and every case asserts
the kernel that ran (e2e_last_kernel)."""
import math

import pytest
import torch
import torch.nn.functional as F

import oracle
from tests.helpers import seeded_input, seeded_labels, structured_kmask, structured_kmask_parts
from tests.test_gpu_ops import _act_value, _eng_stub, _make_act, _plan_and_pack, _prefill, _absmax_word

pytestmark = pytest.mark.gpu

_S1, _S2 = (1, 1, 1), (2, 2, 2)
_CONV_ENTRIES = ("conv133_fwd", "conv133_fwd_sparse", "conv133_fwd_mm", "conv133_fwd_dense", "conv133_fwd_splitk",
                 "conv133_dgrad", "conv133_dgrad_sparse", "conv133_dgrad_mm", "conv133_dgrad_dense", "conv133_dgrad_splitk")
# dispatch notes of the forward and of the data gradient per kernel family (stride-2 plain walk: the sub-pixel form, mode 2)
_NOTES = {"sparse": ("conv133_sparse_kernel<mode=0>", "conv133_sparse_kernel<mode=1>"),
          "plain": ("conv133_kernel<mode=0,", "conv133_kernel<mode=1,"),
          "plain_s2": ("conv133_kernel<mode=0,", "conv133_kernel<mode=2,"),
          "mm": ("conv133_mm_h2<mode=0,", "conv133_mm_h2<mode=1,"),
          "dense": ("conv133_dense_bf3<mode=0>", "conv133_dense_bf3<mode=1>")}


class _KernelLog:
    """e2e_last_kernel() after every call of the conv entry points of the C ABI"""

    def __init__(self, names=_CONV_ENTRIES):
        from e2enet_medical_amd._lib import lib
        self.lib, self.names, self.orig, self.log = lib(), names, {}, []

    def __enter__(self):
        for n in self.names:
            fn = getattr(self.lib, n)
            self.orig[n] = fn

            def wrapped(*a, _fn=fn, _n=n):
                _fn(*a)
                self.log.append((_n, (self.lib.last_kernel() or b"").decode()))
            setattr(self.lib, n, wrapped)
        return self

    def __exit__(self, *exc):
        for n, fn in self.orig.items():
            setattr(self.lib, n, fn)

    def take(self):
        got, self.log = self.log, []
        return got


def _conv_truth(dtype, xs, w, b, gamma, beta, stride, dz=None):
    """conv3d(depth_shift(concat)) -> instance_norm -> leaky_relu and its autograd on the CPU in `dtype`"""
    leaves = [x.to(dtype).clone().requires_grad_(True) for x in xs]
    wl, bl, gl, tl = (t.to(dtype).clone().requires_grad_(True) for t in (w, b, gamma, beta))
    y = F.conv3d(oracle.depth_shift(torch.cat(leaves, 1)), wl, bl, stride=stride, padding=(0, 1, 1))
    y.retain_grad()
    u = F.instance_norm(y, weight=gl, bias=tl, eps=1e-5)
    z = F.leaky_relu(u, 0.01)
    out = dict(y=y.detach(), u=u.detach(), z=z.detach())
    if dz is not None:
        z.backward(dz.to(dtype))
        out.update(dx=[l.grad for l in leaves], dw=wl.grad, db=bl.grad, dgamma=gl.grad, dbeta=tl.grad, dy=y.grad)
    return out


def _per_channel(what, got, r64, r32, bar_of_scale, constant, floor=None):
    """`got` against fp64 per output channel (dim 0), each row at bar_of_scale x that row's own max(1, max |.|) (or at `floor`, a
    per-row absolute bar).  The rows in `constant` -- output planes that are their bias: their gradients are ~316 x the others',
    and so is their fp32 noise, in torch as well -- may miss that bar if over their entries the kernel is no worse than 1.5 x
    torch-fp32's own distance from fp64 (the rule of test_gpu_ops._assert_wgrad).  Returns the worst distance as a fraction of the
    bar over the live rows and over the constant rows, and the two distances the 1.5 x rule compares."""
    C = got.shape[0]
    g, a, b = got.double().reshape(C, -1), r64.double().reshape(C, -1), r32.double().reshape(C, -1)
    e_got, e_32 = (g - a).abs().max(1).values, (b - a).abs().max(1).values
    bar = bar_of_scale * a.abs().max(1).values.clamp(min=1.0) if floor is None else floor
    live, const = [o for o in range(C) if o not in constant], sorted(constant)
    k_const, t_const = (float(e_got[const].max()), float(e_32[const].max())) if const else (0.0, 0.0)
    for o in live:
        assert bool(e_got[o] < bar[o]), "%s, output channel %d: kernel %.3e from fp64, torch fp32 %.3e from fp64, bar %.3e" % (
            what, o, float(e_got[o]), float(e_32[o]), float(bar[o]))
    for o in const:
        assert bool(e_got[o] < bar[o]) or k_const <= 1.5 * t_const, (
            "%s, output channel %d (a constant plane): kernel %.3e from fp64, bar %.3e; over all constant planes: kernel %.3e, "
            "torch fp32 %.3e from fp64" % (what, o, float(e_got[o]), float(bar[o]), k_const, t_const))
    return (float((e_got / bar)[live].max()) if live else 0.0), (float((e_got / bar)[const].max()) if const else 0.0), k_const, t_const


CONV_SHAPES = {
    # path: (B, sources [(C, normed)], Cout, (D,H,W), stride, base density)
    "sparse": (1, [(20, True), (13, False)], 34, (2, 20, 36), _S1, 0.25),
    "sparse_dense_group": (1, [(64, False)], 72, (1, 20, 36), _S1, 0.02),
    "plain": (2, [(20, True), (13, False)], 34, (3, 9, 20), _S1, 0.25),
    "plain_s2": (1, [(12, True), (21, False)], 34, (4, 16, 16), _S2, 0.25),
    "mm": (1, [(20, True), (20, False)], 34, (2, 32, 32), _S1, 0.3),
    "dense": (1, [(20, True), (20, False)], 34, (2, 32, 32), _S1, 0.6),
}
CONV_STRUCTURED_CASES = (
    [("sparse", p) for p in ("dead_rows", "dead_cols", "unused_source", "all_dead")] + [("sparse_dense_group", "dense_group")] +
    [(path, p) for path in ("plain", "plain_s2", "mm") for p in ("dead_rows", "dead_cols", "unused_source")] +
    [("dense", p) for p in ("dead_rows", "dead_cols")])


@pytest.mark.parametrize("shape_key,pattern", CONV_STRUCTURED_CASES)
def test_conv133_structured_masks_vs_fp64(shape_key, pattern, monkeypatch):
    """Conv block forward and backward (normalise-on-load sources, first-writer pass into NaN, then a later-writer pass onto a
    seeded prefill) per kernel family on structured maps, against the fp64 evaluation: the bars of test_conv133_fwd_bwd (2e-5 on y,
    1e-4 on z, 2e-4 of the scale on the gradients), for dw, dgamma, dbeta and db applied PER OUTPUT CHANNEL (a constant plane's
    gradients are ~316 x everyone else's: one global scale would loosen every live row's bar by that factor).  Dead output planes
    get one positive and one negative beta: z = leaky_relu(beta) on them.  The gradient of every dead input plane is exactly 0.0
    after the first-writer pass and bit-identical to the prefill after the later-writer pass."""
    from e2enet_medical_amd import engine as engine_mod
    from e2enet_medical_amd.engine import ConvOp
    from e2enet_medical_amd._lib import lib
    B, src_desc, cout, dims, stride, density = CONV_SHAPES[shape_key]
    path = "sparse" if shape_key.startswith("sparse") else ("plain" if shape_key.startswith("plain") else shape_key)
    cin = sum(c for c, _ in src_desc)
    last = (cin - src_desc[-1][0], cin)                       # unused_source: the last source of the concat
    km = structured_kmask(cout, cin, pattern, seed=5, density=density, col_range=last)
    dead_out, dead_in, _, _ = structured_kmask_parts(cout, cin, pattern, last)
    constant = {o for o in range(cout) if int(km[o].sum()) == 0}
    assert set(dead_out) <= constant and set(dead_in) <= {c for c in range(cin) if int(km[:, c].sum()) == 0}
    if path == "dense":
        # the switch-over densities are tuning thresholds, not limits of the kernels: with the matrix-pipe kernel out of the way
        # (as test_conv133_masks_are_structural_on_every_path does) the bf16x3 dense kernel is next in the dispatch order; the dead
        # rows / columns take the 0.6 map to ~0.47 overall, just under the 0.5 at which a layer is handed to it
        monkeypatch.setattr(engine_mod, "MM_MIN_DENSITY", 2.0)
        monkeypatch.setattr(engine_mod, "DENSE_MIN_DENSITY", 0.4)
    srcs = [_make_act((B, c) + dims, normed, 10 + i) for i, (c, normed) in enumerate(src_desc)]
    w = seeded_input((cout, cin, 1, 3, 3), seed=3) * (1.0 / math.sqrt(cin * 9)) * km.view(cout, cin, 1, 1, 1)
    beta = 0.2 * seeded_input((cout,), seed=7)
    for i, o in enumerate(sorted(constant)):                  # constant planes on both LeakyReLU branches, away from the kink
        beta[o] = (0.05 + 0.01 * (i % 7)) * (1.0 if i % 2 == 0 else -1.0)
    params = {"blk.conv.weight": w, "blk.conv.bias": seeded_input((cout,), seed=4) * 0.1,
              "blk.instnorm.weight": 1 + 0.2 * seeded_input((cout,), seed=6), "blk.instnorm.bias": beta}
    e = _eng_stub(params)
    e.batch = B
    op = ConvOp(e, "blk", srcs, cout, stride)
    if path == "dense":
        assert op.dense_ws_bytes > 0
        e.fwd_ws = torch.empty(op.dense_ws_bytes // 4, dtype=torch.float32, device=e.device)
    rows = torch.empty(((cout + 3) // 4) * ((cin + 7) // 8), dtype=torch.int32, device=e.device)
    cols = torch.empty(((cin + 3) // 4) * ((cout + 7) // 8), dtype=torch.int32, device=e.device)
    lib().dsff_expand_quads(km.to(e.device).data_ptr(), rows.data_ptr(), cols.data_ptr(), cout, cin, 0)
    op.live, op.live_t = rows, cols
    op.density = float(km.float().mean())
    _plan_and_pack(op, km)
    op.set_input_range(max(float(_act_value(a).abs().max()) for a in srcs))
    assert op.path("f") == path and op.path("b") == path, (op.path("f"), op.path("b"), op.density)
    want_f, want_b = _NOTES["plain_s2" if shape_key == "plain_s2" else path]

    xs = [_act_value(a) for a in srcs]
    pnames = ("blk.conv.weight", "blk.conv.bias", "blk.instnorm.weight", "blk.instnorm.bias")
    fwd64 = _conv_truth(torch.float64, xs, *(params[n] for n in pnames), stride)
    dz = seeded_input(tuple(fwd64["z"].shape), seed=8)
    dz[fwd64["u"].abs() < 2e-5] = 0.0                         # (no gradient into elements on the LeakyReLU kink: test_conv133_fwd_bwd)
    t64 = _conv_truth(torch.float64, xs, *(params[n] for n in pnames), stride, dz)
    t32 = _conv_truth(torch.float32, xs, *(params[n] for n in pnames), stride, dz)

    with _KernelLog() as klog:
        # ---- forward
        op.forward()
        torch.cuda.synchronize()
        (entry_f, note_f), = klog.take()
        assert note_f.startswith(want_f), (entry_f, note_f)
        if path == "plain":
            assert note_f.endswith("ksplit=1"), note_f
        if pattern == "dense_group":
            assert note_f.endswith("kmax=256"), note_f       # a fully live 32-plane group: the largest block a chunk can have
        got_y = op.out.data.cpu()
        assert got_y.shape == t64["y"].shape
        err_y = float((got_y.double() - t64["y"]).abs().max())
        z_got = _act_value(op.out)
        err_z = float((z_got.double() - t64["z"]).abs().max())
        print("structured conv %s %s: %s | y %.3e z %.3e from fp64 (torch fp32: %.3e, %.3e)" % (
            shape_key, pattern, note_f, err_y, err_z, float((t32["y"].double() - t64["y"]).abs().max()),
            float((t32["z"].double() - t64["z"]).abs().max())))
        assert err_y < 2e-5, "conv output"
        assert err_z < 1e-4, "normalised output"
        bias = params["blk.conv.bias"]
        for o in sorted(constant):
            assert torch.equal(got_y[:, o], bias[o].expand_as(got_y[:, o])), "an output plane without a live kernel is its bias"
            want = F.leaky_relu(beta[o], 0.01)
            assert float((z_got[:, o] - want).abs().max()) <= 1e-5, ("z of constant plane", o, float(beta[o]))
        if pattern == "all_dead":
            assert torch.equal(got_y, bias.view(1, cout, 1, 1, 1).expand_as(got_y))

        # ---- backward as the first writer of every source gradient
        def backward(written, prefill):
            for s in srcs:
                s._grad_written = written
            op.out.alloc_grad()
            op.plan_backward()
            op.out.grad.copy_(dz)
            for s, p in zip(srcs, prefill):
                s.grad.copy_(p)
            op.backward()
            torch.cuda.synchronize()
            (entry_b, note_b), = klog.take()
            assert note_b.startswith(want_b), (entry_b, note_b)
            return note_b
        note_b = backward(False, [torch.full(s.shape, float("nan")) for s in srcs])
        g = e.grads
        worst = {}
        worst["dw"] = _per_channel("dw", g["blk.conv.weight"].cpu(), t64["dw"], t32["dw"], 2e-4, constant)
        worst["dgamma"] = _per_channel("dgamma", g["blk.instnorm.weight"].cpu(), t64["dgamma"], t32["dgamma"], 2e-4, constant)
        worst["dbeta"] = _per_channel("dbeta", g["blk.instnorm.bias"].cpu(), t64["dbeta"], t32["dbeta"], 2e-4, constant)
        # db is the rounding residue of sum dy (a bias in front of an InstanceNorm has an exactly-zero gradient): it has no maximum
        # of its own to be compared against, and what it scales with is sum |dy| of its plane, not dz.  Per channel: what fp32
        # allows -- dy_i = gamma rstd (du_i - m1 - xhat_i m2) is formed with four roundings (du - m1, xhat m2, the difference, the
        # product; gamma rstd and the stored mean / rstd are common factors of a sum that is exactly zero), m1 = mean du once more
        # over the whole plane, each relative to terms of the size of dy_i / (gamma rstd) unless the xhat m2 term cancels half of
        # it: |db| <= 8 x 2^-24 x sum |dy| -- and never more than the bar of test_conv133_fwd_bwd, 1e-3 max(1, 1e-3 sum |dz|) over
        # the whole of dz (its scale holds no gradient, so no constant plane inflates it).  The first is the smaller one (by 100 x
        # on an ordinary plane) unless |gamma| rstd > ~70 C: on the constant planes the second is.  Measured there, on an MI355X:
        # kernel 7e-4 .. 9.5e-3 from fp64, torch fp32 5e-4 .. 1.5e-2, the ratio of the two between 0.14 and 1.7 from case to case
        # (two roundings of the same size: with the plane's own sum |dz| in the bar, ~1e-3, neither passes).
        db_bar = torch.minimum(8.0 * 2.0 ** -24 * t64["dy"].abs().sum((0, 2, 3, 4)),
                               torch.full((cout,), 1e-3 * max(1.0, float(dz.double().abs().sum()) * 1e-3), dtype=torch.float64))
        worst["db"] = _per_channel("db", g["blk.conv.bias"].cpu(), t64["db"], t32["db"], None, constant, floor=db_bar)
        print("structured conv %s %s: %s | worst of the live rows and of the constant rows as a fraction of the bar, then kernel and "
              "torch fp32 from fp64 over the constant rows: %s" % (
                  shape_key, pattern, note_b, ", ".join("%s %.3f %.3f %.3e %.3e" % ((k,) + v) for k, v in worst.items())))
        c0 = 0
        firsts = []
        for s, ref in zip(srcs, t64["dx"]):
            got = s.grad.cpu()
            firsts.append(got)
            assert torch.isfinite(got).all(), "dgrad left unwritten cells"
            assert float((got.double() - ref).abs().max()) < 2e-4 * max(1.0, float(ref.abs().max())), "dgrad"
            for c in dead_in:
                if c0 <= c < c0 + s.shape[1]:
                    assert bool((got[:, c - c0] == 0.0).all()), "first writer: dead input plane %d is not zero-filled" % c
            if pattern == "all_dead":
                assert bool((got == 0.0).all())
            c0 += s.shape[1]

        # ---- and as a later writer, onto what an earlier consumer left there
        P = [_prefill(s.shape, 900 + i) for i, s in enumerate(srcs)]
        backward(True, P)
        c0 = 0
        for s, ref, p in zip(srcs, t64["dx"], P):
            got = s.grad.cpu()
            want = p.double() + ref
            assert float((got.double() - want).abs().max()) < 2e-4 * max(1.0, float(want.abs().max())), "dgrad accumulate"
            for c in dead_in:
                if c0 <= c < c0 + s.shape[1]:
                    assert torch.equal(got[:, c - c0].view(torch.int32), p[:, c - c0].view(torch.int32)), \
                        "later writer: dead input plane %d was touched" % c
            if pattern == "all_dead":
                assert torch.equal(got.view(torch.int32), p.view(torch.int32))
            c0 += s.shape[1]


def _ct_map(cin, cout, seed, density=0.3):
    """[Cin, Cout] map of a transposed conv: i.i.d., with one dead in-channel, the in-channels of the ragged last 32-word dead
    (Cin = 33: input 32), one dead out-channel and the out-channels of the ragged last 32-word dead (Cout = 40: outputs 32..39) --
    so the second liveness word of every row, in both orientations, is entirely zero."""
    g = torch.Generator().manual_seed(seed)
    km = (torch.rand((cin, cout), generator=g) < density).to(torch.uint8)
    assert cin % 32 and cout % 32
    dead_in = [5] + list(range(32 * (cin // 32), cin))
    dead_out = [7] + list(range(32 * (cout // 32), cout))
    km[dead_in, :] = 0
    km[:, dead_out] = 0
    assert int(km[dead_in].sum()) == 0 and int(km[:, dead_out].sum()) == 0 and int(km.sum()) > 0
    assert int(km[:, 32 * (cout // 32):].sum()) == 0 and int(km[32 * (cin // 32):].sum()) == 0       # the zero liveness words
    return km, dead_in, dead_out


CT_STRUCTURED_CASES = [
    # (B, Cin, Cout, (D,H,W), kernel, range words, forward note, data-gradient note)
    (2, 33, 40, (3, 5, 7), (2, 2, 2), True, "convT_fwd_gather<", "convT_dgrad_gather<8>"),          # the scalar walk
    (1, 72, 40, (8, 32, 32), (2, 2, 2), True, "convT_fwd_h2<4,4>", "convT_dgrad_h2<4>"),            # the split-operand GEMMs: fp16 two-piece
    (1, 72, 40, (8, 32, 32), (2, 2, 2), False, "convT_fwd_bf3<4,4>", "convT_dgrad_bf3<4>"),         # ... and bf16 three-piece
    (2, 33, 40, (8, 32, 34), (1, 2, 2), True, "convT_fwd_gather<", "convT_dgrad_v3<2>"),            # fp32-MFMA data gradient (W % 32 != 0)
]


@pytest.mark.parametrize("case", CT_STRUCTURED_CASES)
def test_convT_structured_masks_vs_fp64(case):
    """Transposed conv (body and bars of test_convT_fwd_bwd, truth in fp64) on a map with a dead in-channel, a dead out-channel and
    a liveness word that is entirely zero: y of a dead out-channel is exactly 0; dx of a dead in-channel is exactly 0 as the first
    writer and untouched as a later writer."""
    from e2enet_medical_amd.engine import UpOp
    from e2enet_medical_amd._lib import lib
    B, cin, cout, dims, kernel, words, want_f, want_b = case
    L = lib()
    src = _make_act((B, cin) + dims, True, 21)
    km, dead_in, dead_out = _ct_map(cin, cout, 23)
    w = seeded_input((cin, cout) + kernel, seed=22) * (1.0 / math.sqrt(cin)) * km.view(cin, cout, 1, 1, 1)
    e = _eng_stub({"up.weight": w})
    op = UpOp(e, "up.weight", src, cout, kernel)
    rows = torch.empty(cin * ((cout + 31) // 32), dtype=torch.int32, device=e.device)
    cols = torch.empty(cout * ((cin + 31) // 32), dtype=torch.int32, device=e.device)
    L.dsff_expand(km.to(e.device).data_ptr(), None, rows.data_ptr(), cols.data_ptr(), cin, cout, 1, 0)
    op.live, op.live_t = cols, rows
    if words:
        op.set_ranges(float(_act_value(src).abs().max()), float(w.abs().max()), 1.0)
    op.forward()
    torch.cuda.synchronize()
    note_f = (L.last_kernel() or b"").decode()
    assert note_f.startswith(want_f), note_f
    x64 = _act_value(src).double().requires_grad_(True)
    w64 = w.double().requires_grad_(True)
    y64 = F.conv_transpose3d(x64, w64, stride=kernel)
    got_y = op.out.data.cpu()
    err_y = float((got_y.double() - y64.detach()).abs().max())
    assert err_y < 2e-5, note_f
    for o in dead_out:
        assert bool((got_y[:, o] == 0.0).all()), "dead out-channel %d" % o
    dy = seeded_input(tuple(y64.shape), seed=24)
    y64.backward(dy.double())

    held = {}

    def backward(written, prefill):
        src._grad_written = written
        op.out.alloc_grad()
        op.plan_backward()
        op.out.grad.copy_(dy)
        if words:
            held["word"] = _absmax_word(op.out.grad)             # max |dy|, as the consuming conv's e2e_in_lrelu_bwd leaves it
            op.dy_word = held["word"].data_ptr()
        src.grad.copy_(prefill)
        op.backward()
        torch.cuda.synchronize()
        note = (L.last_kernel() or b"").decode()
        assert note.startswith(want_b), note
        return src.grad.cpu()
    first = backward(False, torch.full(src.shape, float("nan")))
    err_w = float((e.grads["up.weight"].cpu().double() - w64.grad).abs().max())
    err_x = float((first.double() - x64.grad).abs().max())
    print("structured convT %s: %s | y %.3e dw %.3e (scale %.3g) dx %.3e (scale %.3g)" % (
        case[:6], note_f, err_y, err_w, float(w64.grad.abs().max()), err_x, float(x64.grad.abs().max())))
    assert err_w < 2e-4 * max(1.0, float(w64.grad.abs().max())), "wgrad"
    assert torch.isfinite(first).all() and err_x < 2e-4 * max(1.0, float(x64.grad.abs().max())), "dgrad"
    for c in dead_in:
        assert bool((first[:, c] == 0.0).all()), "first writer: dead in-channel %d is not zero-filled" % c
    P = _prefill(src.shape, 905)
    later = backward(True, P)
    want = P.double() + x64.grad
    assert float((later.double() - want).abs().max()) < 2e-4 * max(1.0, float(want.abs().max())), "dgrad accumulate"
    for c in dead_in:
        assert torch.equal(later[:, c].view(torch.int32), P[:, c].view(torch.int32)), "later writer: dead in-channel %d was touched" % c


# ---- summation accuracy of the load-balanced kernel where the work is concentrated ----------------------------------------------
SUM_CIN, SUM_COUT, SUM_DIMS = 160, 64, (2, 20, 36)


def planned_summation_errors(pattern, flush_every=None):
    """rms distance from the fp64 conv over the heavy planes of `pattern`, for the load-balanced kernel and for torch-CPU fp32, on
    bit-identical operands (one raw source, weights scaled by 1 / sqrt(9 x live fan-in of the row)): heavy_rows / one_heavy_row in
    the forward, heavy_cols / one_heavy_col in the data gradient.  flush_every: None = the plan's own.
    Returns (err_kernel, err_torch, flush_every used, dispatch note)."""
    from e2enet_medical_amd.engine import ConvOp
    from e2enet_medical_amd._lib import lib
    L = lib()
    cin, cout, dims = SUM_CIN, SUM_COUT, SUM_DIMS
    km = structured_kmask(cout, cin, pattern, seed=31)
    _, _, heavy_r, heavy_c = structured_kmask_parts(cout, cin, pattern)
    fan = km.sum(1).clamp(min=1).float()
    w = seeded_input((cout, cin, 1, 3, 3), seed=32) * km.view(cout, cin, 1, 1, 1) / torch.sqrt(9.0 * fan).view(cout, 1, 1, 1, 1)
    src = _make_act((1, cin) + dims, False, 33)
    e = _eng_stub({"blk.conv.weight": w, "blk.conv.bias": torch.zeros(cout), "blk.instnorm.weight": torch.ones(cout),
                   "blk.instnorm.bias": torch.zeros(cout)})
    op = ConvOp(e, "blk", [src], cout, _S1)
    rows = torch.empty(((cout + 3) // 4) * ((cin + 7) // 8), dtype=torch.int32, device=e.device)
    cols = torch.empty(((cin + 3) // 4) * ((cout + 7) // 8), dtype=torch.int32, device=e.device)
    L.dsff_expand_quads(km.to(e.device).data_ptr(), rows.data_ptr(), cols.data_ptr(), cout, cin, 0)
    op.live, op.live_t, op.density = rows, cols, float(km.float().mean())
    op.out.alloc_grad()
    op.plan_backward()
    assert _plan_and_pack(op, km)
    assert op.path("f") == "sparse" and op.path("b") == "sparse"
    x = src.data.cpu()
    forward = bool(heavy_r)
    sp = op.sp_fwd if forward else op.sp_bwd
    if flush_every is not None:
        sp.flush_every = int(flush_every)
    assert 1 <= sp.flush_every <= sp.nchunks

    def rms(a, b, planes):
        return float((a.double()[:, planes] - b[:, planes]).pow(2).mean().sqrt())
    if forward:
        y64 = F.conv3d(oracle.depth_shift(x.double()), w.double(), None, padding=(0, 1, 1))
        y32 = F.conv3d(oracle.depth_shift(x), w, None, padding=(0, 1, 1))
        op.out.data.fill_(float("nan"))
        L.conv133_fwd_sparse(sp.table.data_ptr(), cin, sp.wpk.data_ptr(), e.params["blk.conv.bias"].data_ptr(), sp.quads.data_ptr(),
                             sp.woff.data_ptr(), sp.kmax, sp.qslot.data_ptr(), sp.flush_every, op.out.data.data_ptr(), op.part.data_ptr(),
                             1, cout, *dims, 0)
        torch.cuda.synchronize()
        note = L.last_kernel().decode()
        assert note.startswith("conv133_sparse_kernel<mode=0>") and ("flush=%d " % sp.flush_every) in note, note
        got = op.out.data.cpu()
        return rms(got, y64, heavy_r), rms(y32, y64, heavy_r), sp.flush_every, note
    dy = seeded_input((1, cout) + dims, seed=34)
    xl64 = x.double().requires_grad_(True)
    F.conv3d(oracle.depth_shift(xl64), w.double(), None, padding=(0, 1, 1)).backward(dy.double())
    xl32 = x.clone().requires_grad_(True)
    F.conv3d(oracle.depth_shift(xl32), w, None, padding=(0, 1, 1)).backward(dy)
    op.out.grad.copy_(dy)
    src.grad.fill_(float("nan"))
    L.conv133_dgrad_sparse(op.out.grad.data_ptr(), sp.wpk.data_ptr(), sp.quads.data_ptr(), sp.woff.data_ptr(), sp.kmax, sp.pslot.data_ptr(),
                           op._bwd_table().data_ptr(), None, sp.flush_every, 1, cin, cout, *dims, 0)
    torch.cuda.synchronize()
    note = L.last_kernel().decode()
    assert note.startswith("conv133_sparse_kernel<mode=1>") and ("flush=%d " % sp.flush_every) in note, note
    got = src.grad.cpu()
    assert torch.isfinite(got).all()
    return rms(got, xl64.grad, heavy_c), rms(xl32.grad, xl64.grad, heavy_c), sp.flush_every, note


@pytest.mark.parametrize("pattern", ["heavy_rows", "one_heavy_row", "heavy_cols", "one_heavy_col"])
def test_planned_kernel_summation_on_concentrated_maps(pattern):
    """The two-level summation of conv133_sparse_kernel flushes its chunk accumulators every `flush_every` chunks, an interval the
    plan derives from the map.  Where the work sits in a few output planes (forward: heavy rows; data gradient: heavy columns) the
    heavy planes must stay within 2 x the torch-CPU fp32 conv's rms distance from fp64.  The margin: the project's own record
    (e2e_conv133_sparse_plan, conv133.hip) puts chains of the accepted length at ~1.0-1.27 x the CPU path and single long chains at
    2-6 x, so a factor of 2 separates "two-level summation is working" from "one long chain" without hanging on a seed.
    Measured on an MI355X, kernel / torch (flush_every): with the interval taken from the MEAN live count per plane and chunk, as
    it was until this test, heavy_rows 0.71 (2), one_heavy_row 0.98 (7), heavy_cols 1.36 (2), one_heavy_col 2.33 (8 = never: one
    chain of 576 products); with one flush at the very end 1.76, 1.69, 2.72, 2.33; with the interval taken from the heaviest
    plane (e2e_conv133_sparse_plan now) 0.56, 0.59, 1.03, 0.99, a flush after every chunk in all four."""
    err_k, err_t, flush, note = planned_summation_errors(pattern)
    print("planned summation %s: kernel %.4e, torch fp32 %.4e from fp64 (rms over the heavy planes): ratio %.3f, flush_every %d | %s"
          % (pattern, err_k, err_t, err_k / err_t, flush, note))
    assert err_k <= 2.0 * err_t, (pattern, err_k, err_t, flush)


# ---- one whole network --------------------------------------------------------------------------------------------------------
# width 24 / 48: level 0 (24 and 48 planes of 32 x 32) is served by the load-balanced kernel and by the matrix pipe, and the 48 -> 48
# convs of the deeper levels have too few chunks to be split over workgroups: they stay on the plain walk inside an engine
NET = dict(patch=(8, 32, 32), cin=2, base=24, k=3, pools=[(2, 2, 2), (2, 2, 2), (1, 2, 2), (1, 1, 1), (1, 1, 1)], max_feat=48, B=1)


def _net_maps(names, shapes, layout):
    """per-layer maps of the whole-net case.  layout: weight name -> channels per concat source, for the convs with several
    sources.  Returns (name -> map, name -> (unused source, its first column, one past its last))."""
    kmaps, unused, n_multi, n_single = {}, {}, 0, 0

    def heavy(km):                                           # heavy_rows: every row full or empty
        return bool(((km.sum(1) == 0) | (km.sum(1) == km.shape[1])).all())
    for i, n in enumerate(names):
        r, c = shapes[n][0], shapes[n][1]
        if n in layout and len(layout[n]) > 1:
            which = n_multi % len(layout[n])
            c0 = sum(layout[n][:which])
            unused[n] = (which, c0, c0 + layout[n][which])
            kmaps[n] = structured_kmask(r, c, "unused_source", seed=500 + i, density=0.2, col_range=unused[n][1:])
            n_multi += 1
        elif n.endswith("conv.weight"):
            pat, dens = (("dead_cols", 0.2), ("heavy_rows", None), ("dead_cols", 0.3))[n_single % 3]
            kmaps[n] = structured_kmask(r, c, pat, seed=500 + i, density=dens or 0.25)
            n_single += 1
        else:
            kmaps[n] = structured_kmask(r, c, "dead_cols", seed=500 + i, density=0.3)
        # no output plane loses all its kernels by chance (heavy_rows has such planes by definition): a constant plane puts the
        # fp32 oracle itself 4e-3 of the scale from fp64 on that layer's weight gradient, twice the bar (measured on these maps at
        # base density 0.1); test_conv133_structured_masks_vs_fp64 holds them against fp64.  Such a row gets one kernel back, in a
        # column that has live kernels
        km = kmaps[n]
        if n.endswith("conv.weight") and not heavy(km):
            live_cols = (km.sum(0) > 0).nonzero().flatten()
            for o in (km.sum(1) == 0).nonzero().flatten().tolist():
                km[o, live_cols[o % len(live_cols)]] = 1
            assert bool((km.sum(1) > 0).all())
    return kmaps, unused


def test_whole_net_on_structured_masks(monkeypatch):
    """The recipe of test_whole_net_fixed_seed_sweep (closed-form parameters times the masks, the oracle's loss, logits <= 1e-4 and
    every parameter gradient) with per-layer maps from structured_kmask: unused_source on every conv with more than one source,
    dead_cols and heavy_rows on the others, dead_cols on the transposed convs.  (No dead_rows: constant planes amplify fp32 noise
    through a whole net in the oracle as well; the operator test above covers them.)  The smallest net whose masked convs reach
    the load-balanced kernel, the plain walk and the matrix pipe; with the fused InstanceNorm-backward sums of the planned data
    gradient on (FUSE_IN_SUMS = 2), including for a source none of whose planes has a live kernel."""
    from e2enet_medical_amd import engine as engine_mod
    from tests.test_gpu_net import build_net, load_closed_form
    from tests.test_gpu_configs import _check_all_grads
    monkeypatch.setattr(engine_mod, "FUSE_IN_SUMS", 2)
    N = NET
    net = build_net(N["patch"], N["cin"], N["base"], N["k"], N["pools"], N["max_feat"])
    shapes, params = load_closed_form(net)
    spec = oracle.make_spec(N["cin"], N["base"], N["k"], N["pools"], 2, N["max_feat"])
    names = oracle.masked_names(spec)
    x = seeded_input((N["B"], N["cin"]) + N["patch"], seed=310)
    layout = {n: [s.shape[1] for s in op.sources] for n, op in net.engine(x.cuda()).conv_ops.items()}      # channels per concat source
    net._engines.clear()
    kmaps, unused = _net_maps(names, shapes, layout)
    with torch.no_grad():
        for n in names:
            params[n] = params[n] * kmaps[n].view(kmaps[n].shape + (1, 1, 1)).float()
            net.get_parameter(n).copy_(params[n])
    net.set_kernel_masks(kmaps)
    eng = net.engine(x.cuda())
    outs = eng.forward(x.cuda(), True)
    targets = [seeded_labels((o.shape[0], 1) + tuple(o.shape[2:]), N["k"], seed=400 + i) for i, o in enumerate(outs)]
    wts = oracle.ds_weights(5)
    loss = eng.loss_backward([t.cuda() for t in targets], wts, batch_dice=False)
    paths = {n: (op.path("f"), op.path("b")) for n, op in eng.conv_ops.items() if n in kmaps}
    for n, p in paths.items():
        print("whole net, structured masks: %-40s %-28s density %.3f forward %s, data gradient %s" % (
            n, tuple(kmaps[n].shape), float(kmaps[n].float().mean()), p[0], p[1]))
    reached = {p[0] for p in paths.values()}
    assert {"sparse", "plain", "mm"} <= reached, reached
    fused = [(n, s) for n, op in eng.conv_ops.items() if op.sp_bwd is not None and op.sp_bwd.table is not None for s in op.sp_bwd.fused_srcs]
    fused_unused = [n for n, s in fused if n in unused and eng.conv_ops[n].sources[unused[n][0]] is s]
    print("whole net, structured masks: %d buffers get their InstanceNorm-backward sums from the planned data gradient, %d of them "
          "from a launch that has no live kernel on them (%s)" % (len(fused), len(fused_unused), fused_unused))
    assert fused and fused_unused
    assert all(not op.out.sums_ready for op in eng.conv_ops.values())
    leaves = {n: p.clone().requires_grad_(True) for n, p in params.items()}
    ref = oracle.forward(spec, leaves, x)
    ref_loss = oracle.deep_supervision_loss(ref, targets, wts, False)
    ref_loss.backward()
    for o, r in zip(outs, ref):
        assert (o.cpu() - r.detach()).abs().max() <= 1e-4
    assert abs(loss.item() - ref_loss.item()) < 5e-5
    worst = _check_all_grads(eng, shapes, leaves, tol=2e-3)
    print("whole net, structured masks: worst gradient %.3e of its scale (%s)" % worst)
