"""pld_pgemm_x3_bn_act / pld_pgemm_x3_bn_bwd (csrc/pgemm_x3.hip): the deep-K 1x1 convs of the
MBConv blocks on bf16x3 MFMA with the BN apply / BN backward folded into their operand staging.

Reference per kernel case: the fp32 operand materialised by K.bn_apply / K.bn_bwd, multiplied by
the filter in fp64 on the CPU. Bar: CONV_TOL["bf16x3"] = 1e-4 in test_kernels_gpu.py's rel_err,
for the fused call and for the unfused bf16x3 pair alike.
"""
import numpy as np
import pytest
import torch

from oracle import effnet as OE
from oracle import listmle as LM
from pldepth_amd import kernels as K
from pldepth_amd._lib import PLDError
from pldepth_amd.models.effnet_ff import EffNetFF

pytestmark = pytest.mark.gpu
TOL = 1e-4  # CONV_TOL["bf16x3"]
PAD = 256   # sentinel floats on either side of an output
SENT = -12345.5

# (n, hw, K, N)
CASES = [(3, 57, 144, 40),    # ragged half K-step, N % 32 != 0, rows % strip != 0, strips
                              # straddling images
         (5, 7, 672, 192),    # several images inside one strip
         (1, 20, 480, 80),    # fewer rows than a strip
         (2, 33, 240, 40),
         (2, 100, 672, 112),
         (2, 49, 1152, 192),
         (1, 70, 1152, 320)]  # deepest K and widest N


def rel_err(got, ref):
    got = got.detach().double().cpu()
    ref = ref.detach().double().cpu()
    return float((got - ref).abs().max() / ref.abs().max().clamp(min=1e-30))


def _bn(cuda, g, k):
    mean = torch.randn(k, device=cuda, generator=g) * 0.1
    invstd = torch.rand(k, device=cuda, generator=g) + 0.5
    gamma = torch.rand(k, device=cuda, generator=g) + 0.5
    beta = torch.randn(k, device=cuda, generator=g) * 0.1
    return mean, invstd, gamma, beta


def _unsplit_tile():
    """Index of the plain 64 x 64 bf16x3 im2col tile: one workgroup walks all of K in ascending
    order, the summation order of pgemm_x3."""
    from pldepth_amd import _lib
    n = _lib.lib().pld_conv_num_schedules(K.MATH["bf16x3"])
    return next(t for t in range(n) if K.schedule_desc(K.MATH["bf16x3"], t) == "x3/64x64")


def _guarded(cuda, shape):
    """A tensor of `shape` inside a sentinel-filled buffer, and the buffer."""
    numel = int(np.prod(shape))
    buf = torch.full((numel + 2 * PAD,), SENT, device=cuda)
    return buf[PAD:PAD + numel].view(shape), buf


def _guards_intact(buf):
    return bool((buf[:PAD] == SENT).all()) and bool((buf[-PAD:] == SENT).all())


def _replay_checks(cuda, call, y):
    """A second call and a captured graph replayed twice give the first call's bits."""
    first = y.clone()
    call()
    torch.cuda.synchronize()
    assert torch.equal(y, first)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        gr = K.Graph().capture(call)
        for _ in range(2):
            y.fill_(0.25)
            gr.launch()
            st.synchronize()
            assert torch.equal(y, first)
    torch.cuda.synchronize()


@pytest.mark.parametrize("gate", [True, False])
@pytest.mark.parametrize("n,hw,k,cout", CASES)
def test_pgemm_x3_bn_act(cuda, n, hw, k, cout, gate):
    g = torch.Generator(device=cuda).manual_seed(k + cout + hw)
    rows = n * hw
    x = torch.randn(n, hw, 1, k, device=cuda, generator=g) * 1.5 + 0.2
    bn = _bn(cuda, g, k)
    gt = torch.rand(n, k, device=cuda, generator=g) if gate else None
    wt = torch.randn(1, 1, k, cout, device=cuda, generator=g) / k ** 0.5
    wn = K.filter_to_native(wt)  # [cout][1][1][k]
    K.filter_split(wn)
    a = torch.empty_like(x)
    K.bn_apply(x, rows, k, *bn, "swish", a, gate=gt, hw=hw)
    ref = a.double().cpu().view(rows, k) @ wn.double().cpu().view(cout, k).T
    y_un = torch.empty(n, hw, 1, cout, device=cuda)
    K.conv2d_fwd(K.conv_args(a, None, 1, 1, 1, 0, 0, hw, 1, cout, math="bf16x3"), wn, None, y_un)
    y, buf = _guarded(cuda, (n, hw, 1, cout))
    assert K.pgemm_x3_ok(k, cout)
    call = lambda: K.pgemm_x3_bn_act(x, rows, k, *bn, "swish", wn, cout, y, gate=gt, hw=hw)
    call()
    torch.cuda.synchronize()
    e_f, e_u = rel_err(y.view(rows, cout), ref), rel_err(y_un.view(rows, cout), ref)
    print(f"bn_act {(n, hw, k, cout)} gate {gate}: fused {e_f:.3e} unfused {e_u:.3e}")
    assert e_f < TOL and e_u < TOL, (e_f, e_u)
    assert _guards_intact(buf)
    # the staged operand is bit for bit bn_apply's: on the unsplit tile the pair gives the
    # fused call's bits
    args = K.conv_args(a, None, 1, 1, 1, 0, 0, hw, 1, cout, math="bf16x3")
    args.tile = _unsplit_tile()
    K.conv2d_fwd(args, wn, None, y_un)
    torch.cuda.synchronize()
    assert torch.equal(y, y_un)
    _replay_checks(cuda, call, y)
    # accumulate form: reference + previous contents
    prev = torch.randn(rows, cout, device=cuda, generator=g)
    y.view(rows, cout).copy_(prev)
    K.pgemm_x3_bn_act(x, rows, k, *bn, "swish", wn, cout, y, gate=gt, hw=hw, accumulate=True)
    torch.cuda.synchronize()
    assert rel_err(y.view(rows, cout), ref + prev.double().cpu()) < TOL
    assert _guards_intact(buf)


@pytest.mark.parametrize("n,hw,k,cin", CASES)
def test_pgemm_x3_bn_bwd(cuda, n, hw, k, cin):
    g = torch.Generator(device=cuda).manual_seed(k + cin + hw + 1)
    rows = n * hw
    x = torch.randn(n, hw, 1, k, device=cuda, generator=g) * 1.5 + 0.2
    dy = torch.randn(n, hw, 1, k, device=cuda, generator=g)
    bn = _bn(cuda, g, k)
    w2 = torch.randn(1, 1, cin, k, device=cuda, generator=g) / k ** 0.5
    wd = K.filter_to_dgrad(w2)  # [cin][1][1][k]
    K.filter_split(wd)
    dx_ref = torch.empty_like(x)
    dg_ref, db_ref = torch.empty(k, device=cuda), torch.empty(k, device=cuda)
    K.bn_bwd(x, dy, rows, k, *bn, "swish", dx_ref, dg_ref, db_ref)
    ref = dx_ref.double().cpu().view(rows, k) @ wd.double().cpu().view(cin, k).T
    gx_un = torch.empty(n, hw, 1, cin, device=cuda)
    K.conv2d_dgrad(K.conv_args(gx_un, None, 1, 1, 1, 0, 0, hw, 1, k, math="bf16x3"), dx_ref, wd,
                   gx_un)
    k12 = torch.empty(2 * k, device=cuda)
    dg, db = torch.empty(k, device=cuda), torch.empty(k, device=cuda)
    K.bn_bwd_coeffs(x, dy, rows, k, *bn, "swish", dg, db, k12)
    gx, buf = _guarded(cuda, (n, hw, 1, cin))
    call = lambda: K.pgemm_x3_bn_bwd(x, dy, rows, k, *bn, "swish", k12, wd, cin, gx)
    call()
    torch.cuda.synchronize()
    e_f, e_u = rel_err(gx.view(rows, cin), ref), rel_err(gx_un.view(rows, cin), ref)
    print(f"bn_bwd {(n, hw, k, cin)}: fused {e_f:.3e} unfused {e_u:.3e}")
    assert e_f < TOL and e_u < TOL, (e_f, e_u)
    assert torch.equal(dg, dg_ref) and torch.equal(db, db_ref)
    assert _guards_intact(buf)
    # the staged operand is bit for bit bn_bwd's dx (see test_pgemm_x3_bn_act)
    args = K.conv_args(gx_un, None, 1, 1, 1, 0, 0, hw, 1, k, math="bf16x3")
    args.tile = _unsplit_tile()
    K.conv2d_dgrad(args, dx_ref, wd, gx_un)
    torch.cuda.synchronize()
    assert torch.equal(gx, gx_un)
    _replay_checks(cuda, call, gx)
    prev = torch.randn(rows, cin, device=cuda, generator=g)
    gx.view(rows, cin).copy_(prev)
    K.pgemm_x3_bn_bwd(x, dy, rows, k, *bn, "swish", k12, wd, cin, gx, accumulate=True)
    torch.cuda.synchronize()
    assert rel_err(gx.view(rows, cin), ref + prev.double().cpu()) < TOL
    assert _guards_intact(buf)


def test_pgemm_x3_rejects_unsupported_shapes(cuda):
    assert not K.pgemm_x3_ok(40, 40)      # K % 16 != 0
    assert not K.pgemm_x3_ok(144, 324)    # N above the limit
    assert K.pgemm_x3_ok(1152, 320)
    for k, nn in [(40, 40), (144, 324)]:
        x = torch.zeros(4, k, device=cuda)
        v = torch.ones(k, device=cuda)
        w = torch.zeros(nn, k, device=cuda)
        K.filter_split(w)
        y = torch.zeros(4, nn, device=cuda)
        with pytest.raises(PLDError):
            K.pgemm_x3_bn_act(x, 4, k, v, v, v, v, "swish", w, nn, y)
        with pytest.raises(PLDError):
            K.pgemm_x3_bn_bwd(x, x, 4, k, v, v, v, v, "swish", torch.zeros(2 * k, device=cuda),
                              w, nn, y)


# ------------------------------------------------------------------------------ engine
def _rankings(rng, B, H, W, R, L):
    idx = rng.integers(0, H * W, (B, R, L))
    lab = rng.permutation(B * R * L).reshape(B, R, L) / (B * R * L)
    lab = -np.sort(-lab, axis=-1)
    return np.ascontiguousarray(np.stack([idx.astype(np.float32), lab.astype(np.float32)], -1))


def _structural_zero(name):
    return ((name.startswith("dec_conv") and name.endswith("/bias"))
            or name.endswith("project_bn/beta"))


TAPS = ["block5c_output", "top_activation"]


@pytest.fixture(scope="module")
def engine_errors(cuda, fixed_schedules):
    """One forward + backward of the 64 x 64, batch-2 bf16x3 engine (drop-connect off) with
    pgemm_x3 on every eligible block ("all") and one with it off ("0"), each against the fp64
    oracle: {mode: {tap / "pred" / "grads": error}} and the pgemm_x3 call counts."""
    B, H, R, L = 2, 64, 12, 5
    eng = EffNetFF((H, H, 3), B, seed=0, conv_math="bf16x3")
    eng.drop_connect = False
    rng = np.random.default_rng(0)
    x = rng.random((B, H, H, 3)).astype(np.float32)
    y = _rankings(rng, B, H, H, R, L)
    weights = eng.get_weights()
    calls = {"fwd": 0, "bwd": 0}
    f_act, f_bwd = K.pgemm_x3_bn_act, K.pgemm_x3_bn_bwd

    def count(key, fn):
        def w(*a, **k):
            calls[key] += 1
            return fn(*a, **k)
        return w

    K.pgemm_x3_bn_act, K.pgemm_x3_bn_bwd = count("fwd", f_act), count("bwd", f_bwd)
    runs = {}
    try:
        for mode in ("all", "0"):
            eng.fuse_pgemm_x3 = mode
            calls["fwd"] = calls["bwd"] = 0
            eng.act["input"].copy_(torch.from_numpy(x))
            pred = eng.forward(training=True)
            _, dpred, _ = K.listmle_fwd_bwd(pred, torch.from_numpy(y).to(cuda), B, R, L)
            eng.backward(dpred)
            torch.cuda.synchronize()
            runs[mode] = dict(pred=pred.clone(), taps={t: eng.tap(t).clone() for t in TAPS},
                              grads={k: eng.grads[k].clone() for k in eng.params.names()},
                              calls=dict(calls))
    finally:
        K.pgemm_x3_bn_act, K.pgemm_x3_bn_bwd = f_act, f_bwd
    P = {k: torch.tensor(v, dtype=torch.float64) for k, v in weights.items()}
    x64 = torch.tensor(x, dtype=torch.float64)
    taps = {}
    with torch.no_grad():
        pred_ref = OE.forward(P, x64, taps=taps)
    _, dpred_ref = LM.hourglass_nll(y, pred_ref.numpy(), B, L)
    grads_ref, _ = OE.train_step_grads(P, x64, torch.tensor(dpred_ref))
    keys = [k for k in grads_ref if not _structural_zero(k)]
    flat = lambda gr: torch.cat([gr[k].detach().double().cpu().flatten() for k in keys])
    b = flat(grads_ref)
    err = {}
    for mode, r in runs.items():
        e = {t: rel_err(r["taps"][t], taps[t].permute(0, 2, 3, 1)) for t in TAPS}
        e["pred"] = rel_err(r["pred"], pred_ref)
        e["grads"] = float((flat(r["grads"]) - b).norm() / b.norm())
        err[mode] = e
    for name in TAPS + ["pred", "grads"]:
        print(f"{name}: fused {err['all'][name]:.3e} unfused {err['0'][name]:.3e}")
    return err, {m: r["calls"] for m, r in runs.items()}


def test_engine_runs_fused_path(engine_errors):
    """3a..7a project convs (13) and 3b..7a expand dgrads (12) take pgemm_x3 when it is on, none
    when it is off."""
    _, calls = engine_errors
    assert calls["all"] == {"fwd": 13, "bwd": 12}, calls
    assert calls["0"] == {"fwd": 0, "bwd": 0}, calls


@pytest.mark.parametrize("name", TAPS + ["pred"])
def test_engine_forward_error(engine_errors, name):
    """Per compared tap: the fused error against the fp64 oracle is at most 2 x the unfused
    error + 1e-3 (measured: block5c_output 4.98e-5, top_activation 4.55e-4, pred 1.04e-4 for
    both)."""
    err, _ = engine_errors
    assert err["all"][name] <= 2.0 * err["0"][name] + 1e-3, (name, err)


def test_engine_gradient_error(engine_errors):
    """Global rel-L2 of the non-structural-zero gradients against the fp64 oracle: fused at most
    2 x unfused + 1e-3 (the form of test_model_gpu.py::test_trainable_gradients). Measured on
    MI355X: 2.543e-3 for both (the fused step reproduces the unfused step's bits)."""
    err, _ = engine_errors
    assert err["all"]["grads"] <= 2.0 * err["0"]["grads"] + 1e-3, err
