"""The stride-1 depthwise dgrad with the MBConv block BN's backward applied as its window is
staged and the expand BN's backward sums gathered as its result is stored
(pld_se_bwd_bn_coeffs + pld_dwconv_dgrad_se_bn) against the sequence it replaces:
pld_se_bwd_bn_full (dx) -> pld_dwconv_dgrad -> pld_bn_bwd_coeffs."""
import numpy as np
import pytest
import torch

from pldepth_amd import _lib
from pldepth_amd import kernels as K

pytestmark = pytest.mark.gpu

# (n, h, w, c, k, pt, pl), stride 1
SHAPES = [
    (1, 9, 10, 48, 5, 2, 2),       # map smaller than a tile; c % 32 == 16: half-full last group
    (2, 13, 11, 96, 3, 1, 1),      # two images (per-image gate / addn); ragged tile rows / columns
    (3, 28, 28, 144, 3, 1, 1),     # two tile columns; half-full group
    (4, 28, 28, 1152, 5, 2, 2),    # 36 channel groups: several tiles per workgroup, runs that
                                   # cross image boundaries
    (2, 14, 12, 1152, 3, 1, 1),    # the 14^2 stage
]


def rel_err(got, ref):
    got = got.detach().double().cpu()
    ref = ref.detach().double().cpu()
    return float((got - ref).abs().max() / ref.abs().max().clamp(min=1e-30))


def _bn_vectors(c, cuda, g):
    mean = torch.randn(c, device=cuda, generator=g) * 0.2
    invstd = torch.rand(c, device=cuda, generator=g) + 0.5
    gamma = torch.randn(c, device=cuda, generator=g)
    beta = torch.randn(c, device=cuda, generator=g) * 0.1
    return mean, invstd, gamma, beta


@pytest.mark.parametrize("acc", [False, True])
@pytest.mark.parametrize("n,h,w,c,k,pt,pl", SHAPES)
def test_dwconv_dgrad_se_bn(cuda, n, h, w, c, k, pt, pl, acc):
    g = torch.Generator(device=cuda).manual_seed(c + k + n)
    cse = max(1, c // 24)
    rows = n * h * w
    gse = torch.randn(n, h, w, c, device=cuda, generator=g)
    dw_pre = torch.randn(n, h, w, c, device=cuda, generator=g) * 2 + 0.3
    ex = torch.randn(n, h, w, c, device=cuda, generator=g) * 2 + 0.3
    wdw = torch.randn(k, k, c, device=cuda, generator=g) / k
    bn, ebn = _bn_vectors(c, cuda, g), _bn_vectors(c, cuda, g)
    gate = torch.rand(n, c, device=cuda, generator=g) * 0.98 + 0.01
    z1 = torch.randn(n, cse, device=cuda, generator=g)
    w1 = torch.randn(c, cse, device=cuda, generator=g) * 0.2
    w2 = torch.randn(cse, c, device=cuda, generator=g) * 0.2
    pre = torch.randn(n, h, w, c, device=cuda, generator=g)
    new = lambda *s: torch.empty(*s, device=cuda)

    # the shipped sequence
    addn_ref, dx_ref, dg_ref, db_ref = new(n, c), new(n, h, w, c), new(c), new(c)
    K.se_bwd_bn_full(gse, dw_pre, bn, w1, w2, z1, gate, addn_ref, dx_ref, dg_ref, db_ref)
    ge_ref = pre.clone()
    K.dwconv_dgrad(dx_ref, wdw, k, 1, pt, pl, ge_ref, accumulate=acc)
    edg_ref, edb_ref, ek12_ref = new(c), new(c), new(2 * c)
    K.bn_bwd_coeffs(ex, ge_ref, rows, c, *ebn, "swish", edg_ref, edb_ref, ek12_ref)
    edx_ref = new(n, h, w, c)
    K.bn_bwd(ex, ge_ref, rows, c, *ebn, "swish", edx_ref, new(c), new(c))

    def fused(with_epi):
        addn, dg, db, bk12 = new(n, c), new(c), new(c), new(2 * c)
        K.se_bwd_bn_coeffs(gse, dw_pre, bn, w1, w2, z1, gate, addn, dg, db, bk12)
        ge = pre.clone()
        edg, edb, ek12, edx = new(c), new(c), new(2 * c), new(n, h, w, c)
        if with_epi:
            K.dwconv_dgrad_se_bn(gse, dw_pre, bn, bk12, gate, addn, wdw, k, pt, pl, ge, ex=ex,
                                 ebn=ebn, edgamma=edg, edbeta=edb, ek12=ek12, edx=edx,
                                 accumulate=acc)
        else:
            K.dwconv_dgrad_se_bn(gse, dw_pre, bn, bk12, gate, addn, wdw, k, pt, pl, ge,
                                 accumulate=acc)
        torch.cuda.synchronize()
        return addn, dg, db, ge, edg, edb, ek12, edx

    out = fused(True)
    addn, dg, db, ge, edg, edb, ek12, edx = out
    # the block BN's coefficients come from the same kernels; the staged gradient is the dx
    # bn_bwd_apply_kernel writes, so the dgrad sums the same numbers in the same order
    assert torch.equal(addn, addn_ref) and torch.equal(dg, dg_ref) and torch.equal(db, db_ref)
    assert torch.equal(ge, ge_ref), rel_err(ge, ge_ref)
    # the expand BN's sums: another fixed summation order (test_dwconv_dgrad_bn_bwd's bar)
    for a, r in ((edg, edg_ref), (edb, edb_ref), (ek12, ek12_ref)):
        print("expand BN rel_err", rel_err(a, r))
        assert rel_err(a, r) < 1e-5, rel_err(a, r)
    assert rel_err(edx, edx_ref) < 1e-5, rel_err(edx, edx_ref)
    # the prologue alone (block 1a has no expand conv)
    assert torch.equal(fused(False)[3], ge_ref)
    # graph replays: a second call gives the same bits
    for a, b in zip(out, fused(True)):
        assert torch.equal(a, b)


def test_dwconv_dgrad_se_bn_refuses_other_layers(cuda):
    """Layers the LDS-tiled kernel does not take (c % 16 != 0) are an error, not another kernel:
    the caller runs the unfused pair."""
    n, h, w, c, k = 1, 6, 6, 40, 3
    t = lambda *s: torch.zeros(*s, device=cuda)
    bn = (t(c), t(c), t(c), t(c))
    with pytest.raises(_lib.PLDError):
        K.dwconv_dgrad_se_bn(t(n, h, w, c), t(n, h, w, c), bn, t(2 * c), t(n, c), t(n, c),
                             t(k, k, c), k, 1, 1, t(n, h, w, c))


def test_effnet_backward_fused_matches_unfused(cuda, fixed_schedules):
    """EffNetFF at 64^2, batch 2: one eager backward with the fused depthwise dgrad on (the
    per-block default, then the prologue on every eligible block) and one with it off. The
    prologue stages the bits the unfused apply pass writes, so those gradients are equal."""
    from pldepth_amd.models.effnet_ff import EffNetFF
    eng = EffNetFF((64, 64, 3), 2, seed=0)
    rng = np.random.default_rng(0)
    eng.act["input"].copy_(torch.from_numpy(rng.random((2, 64, 64, 3)).astype(np.float32)))
    dpred = torch.from_numpy(rng.standard_normal((2, 64, 64, 1)).astype(np.float32)).to(cuda)

    def grads(mode):
        eng.fuse_dw_dgrad = mode
        eng.grads.buf.zero_()
        eng.forward(training=True, step=0)
        eng.backward(dpred)
        torch.cuda.synchronize()
        return {name: eng.grads[name].clone() for name in eng.grads.names()}

    ref = grads("0")
    for mode in ("1", "pro"):
        got = grads(mode)
        worst = max((rel_err(got[name], ref[name]), name) for name in ref)
        print(mode, "worst grad rel_err", worst)
        assert worst[0] < 1e-5, (mode, worst)
