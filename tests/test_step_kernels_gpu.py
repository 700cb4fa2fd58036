"""Direct parity tests of the kernels that end every training step and open every inference pass:
Adam-AMSGrad (pld_adam_amsgrad_dev, pld_adam_amsgrad, pld_step_increment, pld_set_scalar_f32),
ListMLE (pld_listmle_fwd_bwd: all four listmle_kernel<EPL> instances, zero_kernel, mean_kernel)
and inference BN (pld_bn_inference_coeffs, pld_channel_affine_act). Each is compared with a plain
float64 restatement of the same operation (oracle/adam.py, oracle/listmle.py, numpy here).

ADAM TOLERANCE. Max-norm relative error per array, err(a) = max|a - ref| / max|ref|, of the update
dp = p_after - p_before and of m, v, vhat against oracle.adam.adam_amsgrad_step64. No bound is a
fixed number: for each case E32 is computed on the CPU as the error of the float32 oracle
(adam_amsgrad_step) against the float64 one, i.e. the reference's own rounding, and

    m, v, vhat:  4 * E32          dp:  4 * E32 + A(t)
    A(t) = n_ulp * 2^-24 * (b2^t / (2 (1 - b2^t)) + b1^t / (1 - b1^t))

The factor 4 covers the different order of roundings (the compiler contracts m + (g - m) * omb1
and friends into fmas; NumPy rounds every product). A(t) is what an error of n_ulp units in the
last place of the device powf does to alpha = lr sqrt(1 - b2^t) / (1 - b1^t): 1 - b2^t cancels at
small t. The device-scalar entry uses n_ulp = N_ULP_DEVICE = 2: the ROCm HIP math documentation
that states powf's bound could not be consulted when these tests were written, and 2 is the
value agreed on for that case. The host-scalar entry computes alpha with the host powf:
n_ulp = 1. dp is compared, not p: at lr = 1e-4 the update is ~1e-4 of p, and a tolerance on p
would say nothing about it (its E32 is then dominated by the half ulp of p, ~1e-3 of dp).

E32, A(t) and the resulting bounds, as computed on the CPU by _adam_bounds for every case below
(entry d = device scalars, h = host scalars):

  entry       n      t     lr    gs | E32: dp       m       v    vhat |    A(t) | bound: dp       m       v    vhat
  d           1      5   0.01     1 | 1.2e-05 4.6e-08 1.1e-08 1.1e-08 | 1.2e-05 |   5.9e-05 1.8e-07 4.2e-08 4.2e-08
  d           3      5   0.01     1 | 9.2e-06 4.1e-08 3.1e-08 7.3e-09 | 1.2e-05 |   4.9e-05 1.6e-07 1.2e-07 2.9e-08
  d           4      5   0.01     1 | 2.3e-05 3.1e-08 2.3e-08 1.5e-08 | 1.2e-05 |   1.0e-04 1.2e-07 9.2e-08 5.8e-08
  d           5      5   0.01     1 | 1.5e-04 9.6e-08 2.9e-08 5.0e-09 | 1.2e-05 |   6.3e-04 3.9e-07 1.2e-07 2.0e-08
  d        1023      5   0.01     1 | 1.8e-05 4.7e-08 3.0e-08 2.0e-08 | 1.2e-05 |   8.3e-05 1.9e-07 1.2e-07 8.0e-08
  d        1027      5   0.01     1 | 1.5e-05 6.1e-08 3.0e-08 2.0e-08 | 1.2e-05 |   7.3e-05 2.4e-07 1.2e-07 8.0e-08
  d     4195507     10   0.01   0.5 | 7.0e-07 5.1e-08 5.9e-08 3.7e-08 | 6.0e-06 |   8.8e-06 2.1e-07 2.4e-07 1.5e-07
  d        1027      1   0.01     1 | 2.9e-05 4.7e-08 3.0e-08 2.0e-08 | 6.1e-05 |   1.8e-04 1.9e-07 1.2e-07 7.9e-08
  d        1027      1 0.0001     1 | 2.1e-03 4.6e-08 4.0e-08 2.0e-08 | 6.1e-05 |   8.5e-03 1.8e-07 1.6e-07 7.9e-08
  d        1027      2   0.01     1 | 1.7e-05 5.0e-08 3.0e-08 2.0e-08 | 3.0e-05 |   9.8e-05 2.0e-07 1.2e-07 8.0e-08
  d        1027      2 0.0001     1 | 1.5e-03 6.5e-08 3.0e-08 2.0e-08 | 3.0e-05 |   6.1e-03 2.6e-07 1.2e-07 7.9e-08
  d        1027     10   0.01     1 | 3.1e-05 6.2e-08 4.3e-08 2.9e-08 | 6.0e-06 |   1.3e-04 2.5e-07 1.7e-07 1.2e-07
  d        1027     10 0.0001     1 | 1.2e-03 6.7e-08 3.0e-08 2.0e-08 | 6.0e-06 |   4.9e-03 2.7e-07 1.2e-07 8.0e-08
  d        1027   1000   0.01     1 | 1.9e-06 8.0e-08 3.0e-08 2.0e-08 | 3.5e-08 |   7.5e-06 3.2e-07 1.2e-07 8.0e-08
  d        1027   1000 0.0001     1 | 3.3e-04 6.5e-08 4.4e-08 2.0e-08 | 3.5e-08 |   1.3e-03 2.6e-07 1.8e-07 7.9e-08
  d        1027 100000   0.01     1 | 2.8e-06 6.5e-08 3.0e-08 2.0e-08 | 2.1e-51 |   1.1e-05 2.6e-07 1.2e-07 7.9e-08
  d        1027 100000 0.0001     1 | 9.0e-05 6.6e-08 3.0e-08 2.0e-08 | 2.1e-51 |   3.6e-04 2.6e-07 1.2e-07 8.0e-08
  d        1027      3   0.01   0.5 | 6.9e-06 6.4e-08 3.0e-08 2.0e-08 | 2.0e-05 |   4.8e-05 2.6e-07 1.2e-07 7.9e-08
  d        1027      3   0.01  0.25 | 5.0e-05 4.1e-08 3.0e-08 2.0e-08 | 2.0e-05 |   2.2e-04 1.7e-07 1.2e-07 7.9e-08
  h        1027      3   0.01   0.5 | 1.9e-05 5.4e-08 3.0e-08 2.0e-08 | 1.0e-05 |   8.8e-05 2.2e-07 1.2e-07 7.8e-08
  h        1027      3   0.01  0.25 | 1.9e-05 5.4e-08 3.0e-08 2.0e-08 | 1.0e-05 |   8.8e-05 2.1e-07 1.2e-07 7.9e-08
  h        1027      1   0.01     1 | 1.2e-05 4.4e-08 3.0e-08 2.0e-08 | 3.0e-05 |   7.8e-05 1.8e-07 1.2e-07 8.0e-08
  h        1029   1000 0.0001     1 | 7.3e-04 6.4e-08 3.0e-08 2.0e-08 | 1.7e-08 |   2.9e-03 2.6e-07 1.2e-07 8.0e-08

LISTMLE TOLERANCE. 1e-5 max-norm relative on loss, per-list nll and dpred, the suite's existing
bound: the float32 NumPy restatement of the oracle formula is within 1.6e-7 (nll) and 2.6e-6
(gradient) of the float64 oracle at every list length and logit spread used here (worst at
L = 512, logits x5). Exact-zero claims (invalid elements, pixels no list names, out-of-range
indices) are asserted as exact zeros. Every call gets dpred, nll and loss pre-filled with NaN.

INFERENCE BN TOLERANCE. 1e-6 on the coefficients (a division, a square root, one fma) and the BN
tests' 1e-5 on act(x * scale + shift), both max-norm relative against float64.
"""
import numpy as np
import pytest
import torch

from oracle import listmle as LM
from oracle.adam import adam_amsgrad_step, adam_amsgrad_step64
from pldepth_amd import kernels as K
from pldepth_amd._lib import PLDError

pytestmark = pytest.mark.gpu

B1, B2, EPS = 0.9, 0.999, 1e-7
N_ULP_DEVICE = 2  # powf's documented bound could not be consulted: 2 stands in (see the header)
N_ULP_HOST = 1
GRID_STRIDE_N = 4096 * 256 * 4 + 4 * 300 + 3  # n4 > 4096 * 256: the float4 loop iterates


def err(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300))


def dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


# ====================================================================================== Adam
def _adam_state(n, t, seed):
    """p, g ~ N(0, 1); m zero at t = 1; vhat above v on about half the elements and below it on
    the rest, so both arms of the kernel's fmaxf are taken in one call."""
    rng = np.random.default_rng(seed)
    p = rng.standard_normal(n).astype(np.float32)
    g = rng.standard_normal(n).astype(np.float32)
    m = (np.zeros(n) if t == 1 else 0.1 * rng.standard_normal(n)).astype(np.float32)
    v = rng.random(n).astype(np.float32)
    vh = (v * np.where(rng.random(n) < 0.5, 1.5, 0.5)).astype(np.float32)
    return p, g, m, v, vh


def _amp(t):
    b1t, b2t = np.float64(np.float32(B1)) ** t, np.float64(np.float32(B2)) ** t
    return float(2.0 ** -24 * (b2t / (2 * (1 - b2t)) + b1t / (1 - b1t)))


def _adam_bounds(state, t, lr, gs, n_ulp):
    """(float64 reference (dp, m, v, vhat), E32 per array, A(t), bound per array) — CPU only."""
    p = state[0].astype(np.float64)
    r64 = adam_amsgrad_step64(*state, lr=lr, step=t, grad_scale=gs)
    r32 = adam_amsgrad_step(*state, lr=lr, step=t, grad_scale=gs)
    ref = (r64[0] - p,) + tuple(r64[1:])
    f32 = (r32[0].astype(np.float64) - p,) + tuple(r32[1:])
    e32 = [err(a, b) for a, b in zip(f32, ref)]
    a_t = n_ulp * _amp(t)
    return ref, e32, a_t, [4 * e32[0] + a_t] + [4 * e for e in e32[1:]]


def _adam_run(cuda, entry, state, t, lr, gs):
    tp, tg, tm, tv, th = (dev(a, cuda) for a in state)
    if entry == "d":
        lr_dev = torch.zeros(1, device=cuda)
        K.set_scalar(lr_dev, lr)
        step_dev = torch.full((1,), t, dtype=torch.int64, device=cuda)
        K.adam_amsgrad_dev(tp, tg, tm, tv, th, lr_dev, step_dev, B1, B2, EPS, grad_scale=gs)
    else:
        K.adam_amsgrad(tp, tg, tm, tv, th, lr, t, B1, B2, EPS, grad_scale=gs)
    torch.cuda.synchronize()
    assert torch.equal(tg.cpu(), torch.from_numpy(state[1])), "the gradient is read-only"
    return [a.cpu().numpy() for a in (tp, tm, tv, th)]


# (entry, n, t, lr, grad_scale)
ADAM_CASES = (
    # sizes: below one float4, ragged tails, and the grid-stride loop with a ragged tail
    [("d", n, 5, 0.01, 1.0) for n in (1, 3, 4, 5, 1023, 1027)]
    + [("d", GRID_STRIDE_N, 10, 0.01, 0.5)]
    # steps x learning rates through step_dev / lr_dev
    + [("d", 1027, t, lr, 1.0) for t in (1, 2, 10, 1000, 100000) for lr in (0.01, 1e-4)]
    # grad_scale on both entries; the host entry also at t = 1 and a late step
    + [(e, 1027, 3, 0.01, gs) for e in ("d", "h") for gs in (0.5, 0.25)]
    + [("h", 1027, 1, 0.01, 1.0), ("h", 1029, 1000, 1e-4, 1.0)]
)
# the same (n, t, lr, gs) appears once per entry at most; seeds are the case's position
assert len(set(ADAM_CASES)) == len(ADAM_CASES)


@pytest.mark.parametrize("case", range(len(ADAM_CASES)),
                         ids=["%s-n%d-t%d-lr%g-gs%g" % c for c in ADAM_CASES])
def test_adam_matches_float64_oracle(cuda, case):
    entry, n, t, lr, gs = ADAM_CASES[case]
    state = _adam_state(n, t, seed=case)
    ref, e32, a_t, bound = _adam_bounds(state, t, lr, gs,
                                        N_ULP_DEVICE if entry == "d" else N_ULP_HOST)
    got = _adam_run(cuda, entry, state, t, lr, gs)
    got[0] = got[0].astype(np.float64) - state[0].astype(np.float64)
    assert all(np.isfinite(a).all() for a in got)
    errs = [err(a, b) for a, b in zip(got, ref)]
    print("adam %s n=%d t=%d lr=%g gs=%g  err %s  E32 %s  A %.3g  bound %s" % (
        entry, n, t, lr, gs, *(" ".join("%.3g" % x for x in xs) for xs in (errs, e32)), a_t,
        " ".join("%.3g" % x for x in bound)))
    for name, e, b in zip(("dp", "m", "v", "vhat"), errs, bound):
        assert e <= b, (name, e, b)
    if n >= 1023:  # both arms of max(vhat, v)
        took_v = ref[3] > state[4]
        assert took_v.any() and (~took_v).any()


SENTINEL = (1234.5, -77.25, 3.0e7, -5.0e-3, 0.125)


@pytest.mark.parametrize("lo,hi", [(16, 16 + 1027), (32, 32 + 5), (0, 4)])
def test_adam_on_a_slice_writes_nothing_outside_it(cuda, lo, hi):
    """trainer._dp_update runs the kernel on buf[lo:hi] of the flat buffers: the float4 body and
    the scalar tail of a slice stay inside [lo, hi) in all four written arrays."""
    total, n, t, lr, gs = 4096 + 64, hi - lo, 7, 0.01, 0.5
    state = _adam_state(n, t, seed=lo)
    bufs = []
    for a, s in zip(state, SENTINEL):
        full = np.full(total, s, np.float32)
        full[lo:hi] = a
        bufs.append(dev(full, cuda))
    lr_dev = torch.full((1,), lr, device=cuda)
    step_dev = torch.full((1,), t, dtype=torch.int64, device=cuda)
    K.adam_amsgrad_dev(*(b[lo:hi] for b in bufs), lr_dev, step_dev, B1, B2, EPS, grad_scale=gs)
    torch.cuda.synchronize()
    out = [b.cpu().numpy() for b in bufs]
    for a, s in zip(out, SENTINEL):
        outside = np.concatenate([a[:lo], a[hi:]])
        assert np.array_equal(outside.view(np.int32),
                              np.full(total - n, s, np.float32).view(np.int32))
    assert np.array_equal(out[1][lo:hi], state[1])
    ref, _, _, bound = _adam_bounds(state, t, lr, gs, N_ULP_DEVICE)
    got = [out[0][lo:hi].astype(np.float64) - state[0]] + [out[k][lo:hi] for k in (2, 3, 4)]
    for name, a, r, b in zip(("dp", "m", "v", "vhat"), got, ref, bound):
        assert err(a, r) <= b, (name, err(a, r), b)


@pytest.mark.parametrize("entry", ["d", "h"])
@pytest.mark.parametrize("t", [1, 100000])
def test_adam_padding_slots_stay_put(cuda, entry, t):
    """FlatStore pads every tensor to 4 floats with zeros and the update runs over the padding:
    where g = m = v = vhat = 0 the parameter is bit-identical afterwards and nothing is NaN."""
    n = 11
    p, g, m, v, vh = _adam_state(n, t, seed=t)
    pad = np.array([2, 3, 7, 9, 10])  # float4 body and scalar tail
    for a in (g, m, v, vh):
        a[pad] = 0.0
    got = _adam_run(cuda, entry, (p, g, m, v, vh), t, 0.01, 1.0)
    assert all(np.isfinite(a).all() for a in got)
    assert np.array_equal(got[0][pad].view(np.int32), p[pad].view(np.int32))
    for a in got[1:]:
        assert np.array_equal(a[pad], np.zeros(len(pad), np.float32))
    keep = np.setdiff1d(np.arange(n), pad)
    assert (got[0][keep] != p[keep]).any()


def test_adam_rejects_bad_arguments_before_any_launch(cuda):
    n = 64
    state = _adam_state(n + 1, 2, seed=5)
    bufs = [dev(a, cuda) for a in state]
    before = [b.clone() for b in bufs]
    lr_dev = torch.full((1,), 0.01, device=cuda)
    step_dev = torch.full((1,), 2, dtype=torch.int64, device=cuda)
    with pytest.raises(PLDError):
        K.adam_amsgrad(*(b[:n] for b in bufs), 0.01, 0, B1, B2, EPS)  # step 0
    with pytest.raises(PLDError):
        K.adam_amsgrad(*(b[1:] for b in bufs), 0.01, 2, B1, B2, EPS)  # 4-byte offset view
    with pytest.raises(PLDError):
        K.adam_amsgrad_dev(*(b[1:] for b in bufs), lr_dev, step_dev, B1, B2, EPS)
    torch.cuda.synchronize()
    for b, b0 in zip(bufs, before):
        assert torch.equal(b.view(torch.int32), b0.view(torch.int32))
    assert step_dev.item() == 2 and lr_dev.item() == float(np.float32(0.01))


def test_step_increment_and_set_scalar(cuda):
    step = torch.full((1,), 1, dtype=torch.int64, device=cuda)
    for _ in range(3):
        K.step_increment(step)
    assert step.item() == 4
    step.fill_(2 ** 31 - 1)
    K.step_increment(step)
    assert step.dtype == torch.int64 and step.item() == 2 ** 31
    s = torch.full((3,), -1.0, device=cuda)
    for value in (0.01, 1e-4, 1.0 / 3.0, 0.0, 6.25):
        K.set_scalar(s[1:2], value)
        assert s.dtype == torch.float32
        assert s.cpu().numpy().tolist() == [-1.0, float(np.float32(value)), -1.0]


def test_adam_graph_replay_is_bit_identical_to_eager(cuda):
    """[adam_amsgrad_dev, step_increment] captured once (a linear graph) and replayed three times,
    a fresh gradient copied into the captured g buffer before each replay."""
    n, lr, gs = 1027, 0.01, 0.5
    state = _adam_state(n, 2, seed=11)  # non-zero m, both max arms
    rng = np.random.default_rng(12)
    grads = [dev(rng.standard_normal(n).astype(np.float32), cuda) for _ in range(3)]

    def start():
        bufs = [dev(a, cuda) for a in state]
        return bufs, torch.full((1,), lr, device=cuda), \
            torch.full((1,), 1, dtype=torch.int64, device=cuda)

    stream = torch.cuda.Stream(device=cuda)
    eager, lr_e, step_e = start()
    replay, lr_r, step_r = start()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        for g in grads:
            eager[1].copy_(g)
            K.adam_amsgrad_dev(*eager, lr_e, step_e, B1, B2, EPS, grad_scale=gs)
            K.step_increment(step_e)
        graph = K.Graph().capture(lambda: (
            K.adam_amsgrad_dev(*replay, lr_r, step_r, B1, B2, EPS, grad_scale=gs),
            K.step_increment(step_r)))
        for g in grads:
            replay[1].copy_(g)
            graph.launch()
    torch.cuda.synchronize()
    assert step_e.item() == 4 and step_r.item() == 4
    for a, b in zip(eager, replay):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert not torch.equal(replay[0].cpu(), torch.from_numpy(state[0]))
    del graph


# =================================================================================== ListMLE
HW0 = 11 * 13


def _lists(rng, B, HW, R, L, spread=1.0):
    """Inputs as test_kernels_gpu.py::test_listmle_matches_oracle builds them: random pixels,
    tie-free labels in no particular order (the kernel's rank computation does the sorting)."""
    pred = (rng.standard_normal((B, HW)) * spread).astype(np.float32)
    idx = rng.integers(0, HW, (B, R, L))
    lab = (rng.permutation(B * R * L).reshape(B, R, L) / (B * R * L)).astype(np.float32)
    return pred, idx.astype(np.float32), lab


def _y(idx, lab):
    return np.ascontiguousarray(np.stack([idx, lab], -1).astype(np.float32))


def _listmle(cuda, pred, y, zero_dpred=True, prior=None):
    B, R, L = y.shape[:3]
    tp = dev(pred, cuda)
    dpred = (torch.full_like(tp, float("nan")) if prior is None else dev(prior, cuda))
    nll = torch.full((B * R,), float("nan"), device=cuda)
    loss = torch.full((1,), float("nan"), device=cuda)
    out = K.listmle_fwd_bwd(tp, dev(y, cuda), B, R, L, dpred=dpred, nll=nll, loss=loss,
                            zero_dpred=zero_dpred)
    torch.cuda.synchronize()
    assert out[0] is loss and out[1] is dpred and out[2] is nll
    return loss.item(), dpred.cpu().numpy(), nll.cpu().numpy()


def _named(y, HW):
    """[B, HW] mask of the pixels that some valid element with an in-range index names."""
    B = y.shape[0]
    tr = np.trunc(y[..., 0].astype(np.float64)).reshape(B, -1)
    ok = (tr >= 0) & (tr < HW) & (y[..., 1].reshape(B, -1) >= 0)
    named = np.zeros((B, HW), bool)
    for b in range(B):
        named[b, tr[b][ok[b]].astype(np.int64)] = True
    return named


def _check_listmle(cuda, pred, y, out_of_range=False, tag=""):
    B, R, L = y.shape[:3]
    loss_ref, dpred_ref, nll_ref = LM.hourglass_nll(y, pred, B, L, return_nll=True,
                                                    out_of_range_zero=out_of_range)
    loss, dpred, nll = _listmle(cuda, pred, y)
    assert np.isfinite(dpred).all() and np.isfinite(nll).all() and np.isfinite(loss)
    # (L = 1: nll = log(e^0) - 0 and its gradient are exactly 0 in any arithmetic; err() then
    # accepts only an exact 0)
    e = (abs(loss - loss_ref) / max(abs(loss_ref), 1e-300), err(nll, nll_ref),
         err(dpred, dpred_ref))
    print("listmle %s B=%d R=%d L=%d HW=%d  err loss %.3g nll %.3g dpred %.3g" % (
        tag, B, R, L, pred.shape[1], *e))
    assert max(e) < 1e-5, (tag, e)
    # a pixel no list names (or only invalid and out-of-range elements name) is exactly zero
    named = _named(y, pred.shape[1])
    assert np.array_equal(dpred[~named], np.zeros(int((~named).sum()), np.float32))
    return dpred, nll, dpred_ref, named


@pytest.mark.parametrize("L", [1, 2, 63, 64, 65, 100, 128, 129, 256, 257, 511, 512])
def test_listmle_every_instance_and_boundary(cuda, L):
    """L <= 64, 128, 256, 512 select listmle_kernel<1, 2, 4, 8>; B * R = 1, 2, 3, 5 lists leave
    3, 2, 1, 3 inactive waves in the last block; logits at spread 1 and 5."""
    rng = np.random.default_rng(1000 + L)
    for B, R in ((1, 1), (1, 2), (3, 1), (1, 5)):
        for spread in (1.0, 5.0):
            pred, idx, lab = _lists(rng, B, HW0, R, L, spread)
            _check_listmle(cuda, pred, _y(idx, lab), tag="x%g" % spread)


def test_listmle_more_lists_than_the_mean_kernel_has_threads(cuda):
    rng = np.random.default_rng(300)
    pred, idx, lab = _lists(rng, 3, HW0, 100, 5)
    _check_listmle(cuda, pred, _y(idx, lab))


@pytest.mark.parametrize("L", [40, 100, 200, 400])
@pytest.mark.parametrize("pattern", ["front", "middle", "last_third", "whole_list"])
def test_listmle_invalid_labels(cuda, L, pattern):
    """Label -1 marks an element invalid: it stays in the list at logit log(1e-10), sorts last,
    and gets exactly 0.0 gradient. Every pixel is named once, so its gradient is its element's."""
    rng = np.random.default_rng(L)
    B, R = 2, 3
    HW = R * L + 7
    for spread in (1.0, 5.0):
        pred, _, lab = _lists(rng, B, HW, R, L, spread)
        idx = np.stack([rng.permutation(HW)[:R * L] for _ in range(B)]).reshape(B, R, L)
        if pattern == "front":
            lab[:, :, 0] = -1.0
        elif pattern == "middle":
            lab[:, :, [L // 3, L // 2, L // 2 + 1, 2 * L // 3]] = -1.0
        elif pattern == "last_third":
            lab[:, :, L - L // 3:] = -1.0
        else:
            lab[0, 1] = -1.0
            lab[1, 2] = -1.0
        y = _y(idx.astype(np.float32), lab)
        dpred, nll, _, _ = _check_listmle(cuda, pred, y, tag=pattern + " x%g" % spread)
        for b in range(B):
            bad = idx[b][lab[b] < 0]
            assert bad.size and np.array_equal(dpred[b, bad], np.zeros(bad.size, np.float32))
        if pattern == "whole_list":  # every logit equal: nll = log(L!)
            want = np.sum(np.log(np.arange(1, L + 1)))
            assert abs(nll[1] - want) < 1e-5 * want and abs(nll[R + 2] - want) < 1e-5 * want


@pytest.mark.parametrize("L", [5, 70, 130, 300])
def test_listmle_unsorted_ties(cuda, L):
    """Labels from 4 levels, in no order: among equal labels the later element goes first, in the
    kernel's rank computation and in the oracle's stable sort alike."""
    rng = np.random.default_rng(L)
    B, R = 2, 3
    pred, idx, _ = _lists(rng, B, HW0, R, L)
    lab = (rng.integers(0, 4, (B, R, L)) / 4.0).astype(np.float32)
    lab[1, 0, L // 2] = -1.0  # ties with the minimum level's invalid score never arise: -1e-6
    _check_listmle(cuda, pred, _y(idx, lab))


@pytest.mark.parametrize("L", [6, 100, 400])
def test_listmle_duplicate_pixels_accumulate(cuda, L):
    rng = np.random.default_rng(L)
    HW = 2 * L + 3
    # list 0: every entry names pixel 5; lists 1 and 2 share the first half of their pixels
    pred, idx, lab = _lists(rng, 1, HW, 3, L)
    idx[0, 0, :] = 5.0
    own = rng.permutation(HW)[:2 * L].astype(np.float32)
    idx[0, 1] = own[:L]
    idx[0, 2, :L // 2] = own[:L // 2]
    idx[0, 2, L // 2:] = own[L:L + L - L // 2]
    dpred, _, ref, _ = _check_listmle(cuda, pred, _y(idx, lab))
    shared = own[:L // 2].astype(int)
    assert (np.abs(ref[0, shared]) > 0).all()
    # second image of the same batch, no duplicates: the two images do not mix
    pred2, idx2, lab2 = _lists(rng, 2, HW, 2, L)
    idx2[0, :, :] = 1.0
    _check_listmle(cuda, pred2, _y(idx2, lab2))


def test_listmle_fractional_indices_truncate(cuda):
    """tf.cast(float32 -> int32) truncates toward zero: 3.7 names pixel 3, -0.5 pixel 0."""
    pred = np.random.default_rng(0).standard_normal((1, 9)).astype(np.float32)
    y = _y(np.array([[[3.7, 5.2, -0.5]]], np.float32), np.array([[[0.3, 0.9, 0.6]]], np.float32))
    dpred, _, _, _ = _check_listmle(cuda, pred, y)
    assert sorted(np.nonzero(dpred[0])[0].tolist()) == [0, 3, 5]
    whole = _listmle(cuda, pred, _y(np.array([[[3.0, 5.0, 0.0]]], np.float32), y[..., 1]))
    frac = _listmle(cuda, pred, y)
    assert whole[0] == frac[0] and np.array_equal(whole[1], frac[1])
    rng = np.random.default_rng(1)
    pred, idx, lab = _lists(rng, 2, HW0, 3, 100)
    _check_listmle(cuda, pred, _y(idx + rng.random(idx.shape).astype(np.float32) * 0.9, lab))


@pytest.mark.parametrize("L", [5, 100, 200, 400])
def test_listmle_out_of_range_indices(cuda, L):
    """An index outside [0, HW) after truncation gathers 0.0 and receives no gradient (the
    kernel's two guards, `ii >= 0 && ii < HW` at the gather and at the scatter); the element
    still takes part in its list."""
    rng = np.random.default_rng(L)
    B, R, HW = 2, 3, 3 * L + 11
    pred, idx, lab = _lists(rng, B, HW, R, L)
    outs = np.array([-1.0, HW, HW + 5, 2.0 ** 31], np.float32)
    for b in range(B):
        for r in range(R):
            where = rng.permutation(L)[:4]
            idx[b, r, where] = outs[:len(where)]
    y = _y(idx, lab)
    # _check_listmle asserts exact zeros on every pixel outside the in-range ones
    dpred, _, ref, named = _check_listmle(cuda, pred, y, out_of_range=True)
    assert (~named).any() and (dpred[named] != 0).any()


@pytest.mark.parametrize("B,HW", [(1, 3), (1, 49), (5, 29), (2, 75)])
def test_listmle_zero_dpred_clears_a_poisoned_buffer(cuda, B, HW):
    """B * HW = 3, 49, 145, 150: no multiple of 4 (3 is below one float4), so zero_kernel's scalar
    tail runs. dpred starts as NaN everywhere (_listmle fills it)."""
    rng = np.random.default_rng(B * HW)
    R, L = (1, 2) if HW == 3 else (2, 5)
    pred, idx, lab = _lists(rng, B, HW, R, L)
    _, _, _, named = _check_listmle(cuda, pred, _y(idx, lab))
    assert (~named).any()  # some pixel is named by no list: exactly 0.0 (_check_listmle)


@pytest.mark.parametrize("B,HW", [(1, 3), (5, 29), (2, 75)])
def test_listmle_accumulates_without_zero_dpred(cuda, B, HW):
    rng = np.random.default_rng(B * HW + 1)
    R, L = (1, 2) if HW == 3 else (2, 5)
    pred, idx, lab = _lists(rng, B, HW, R, L)
    y = _y(idx, lab)
    prior = (0.25 * rng.standard_normal((B, HW))).astype(np.float32)
    loss_ref, dpred_ref = LM.hourglass_nll(y, pred, B, L)
    loss, dpred, _ = _listmle(cuda, pred, y, zero_dpred=False, prior=prior)
    assert abs(loss - loss_ref) < 1e-5 * abs(loss_ref)
    assert err(dpred, prior.astype(np.float64) + dpred_ref) < 1e-5
    untouched = ~_named(y, HW)
    assert untouched.any() and np.array_equal(dpred[untouched], prior[untouched])


def test_per_list_loss_wrapper(cuda):
    """NegativeLogLikelihoodLoss: each list is its own image (HW = L, B = N)."""
    from pldepth_amd.losses.nll_loss import NegativeLogLikelihoodLoss
    rng = np.random.default_rng(79)
    N, L = 7, 9
    s = rng.standard_normal((N, L)).astype(np.float32)
    lab = (rng.permutation(N * L).reshape(N, L) / (N * L)).astype(np.float32)
    lab[2, 4] = -1.0
    loss, g = NegativeLogLikelihoodLoss(L).loss_and_grad(lab, s)
    torch.cuda.synchronize()
    nll_ref, g_ref = LM.listmle_fwd_bwd(s, lab)
    assert tuple(g.shape) == (N, L)
    assert abs(loss.item() - nll_ref.mean()) < 1e-5 * abs(nll_ref.mean())
    assert err(g.cpu().numpy(), g_ref / N) < 1e-5
    assert g[2, 4].item() == 0.0


# ============================================================================== inference BN
ACTS = list(K.ACT)  # every selector the wrapper accepts, aliases of "none" included


def _act64(act, z):
    if act == "relu":
        return np.maximum(z, 0.0)
    if act == "swish":
        return z / (1.0 + np.exp(-z))
    if act == "sigmoid":
        return 1.0 / (1.0 + np.exp(-z))
    assert act in ("none", "linear", None), act
    return z


@pytest.mark.parametrize("c", [3, 6, 32, 144, 1280])
def test_bn_inference_coeffs(cuda, c):
    rng = np.random.default_rng(c)
    gamma, beta, mmean = (rng.standard_normal(c).astype(np.float32) for _ in range(3))
    mvar = (rng.random(c) * 2).astype(np.float32)
    mvar[0], mvar[c // 2] = 0.0, 1e-8
    scale = torch.full((c,), float("nan"), device=cuda)
    shift = torch.full((c,), float("nan"), device=cuda)
    K.bn_inference_coeffs(*(dev(a, cuda) for a in (gamma, beta, mmean, mvar)), scale, shift,
                          eps=1e-3)
    torch.cuda.synchronize()
    eps = np.float64(np.float32(1e-3))
    scale_ref = gamma.astype(np.float64) / np.sqrt(mvar.astype(np.float64) + eps)
    shift_ref = beta.astype(np.float64) - mmean.astype(np.float64) * scale_ref
    assert err(scale.cpu().numpy(), scale_ref) < 1e-6
    assert err(shift.cpu().numpy(), shift_ref) < 1e-6


def _affine_case(rows, c, seed):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((rows, c)) * 2).astype(np.float32)
    scale = ((0.5 + rng.random(c)) * np.where(rng.random(c) < 0.3, -1, 1)).astype(np.float32)
    shift = rng.standard_normal(c).astype(np.float32)
    z = x.astype(np.float64) * scale.astype(np.float64) + shift.astype(np.float64)
    return x, scale, shift, z


@pytest.mark.parametrize("act", ACTS, ids=[str(a) for a in ACTS])
@pytest.mark.parametrize("rows,c", [(50, 6), (999, 144), (301, 3), (1, 4)])
def test_channel_affine_act(cuda, rows, c, act):
    x, scale, shift, z = _affine_case(rows, c, rows * c)
    tx, ts, th = dev(x, cuda), dev(scale, cuda), dev(shift, cuda)
    y = torch.full_like(tx, float("nan"))
    K.channel_affine_act(tx, rows, c, ts, th, act, y)
    torch.cuda.synchronize()
    assert torch.equal(tx.cpu(), torch.from_numpy(x))
    assert err(y.cpu().numpy(), _act64(act, z)) < 1e-5
    K.channel_affine_act(tx, rows, c, ts, th, act, tx)  # in place, as _BN.add_apply uses it
    torch.cuda.synchronize()
    assert torch.equal(tx.view(torch.int32), y.view(torch.int32))


@pytest.mark.parametrize("rows,c", [(30011, 288), (2100007, 3)])
def test_channel_affine_act_grid_stride(cuda, rows, c):
    """More than 8192 * 256 vectors: the grid-stride loop iterates, with the grid trimmed so that
    every thread stays on one channel group (VW = 4 with c / 4 = 72: a multiple of 9 blocks;
    VW = 1 with c = 3: a multiple of 3). Each thread loads its coefficients once, so a wrong
    stride shows as another channel's scale and shift."""
    assert rows * c // (4 if c % 4 == 0 else 1) > 8192 * 256
    x, scale, shift, z = _affine_case(rows, c, c)
    y = torch.full((rows, c), float("nan"), device=cuda)
    K.channel_affine_act(dev(x, cuda), rows, c, dev(scale, cuda), dev(shift, cuda), "swish", y)
    torch.cuda.synchronize()
    got = y.cpu().numpy()
    assert err(got, _act64("swish", z)) < 1e-5
    assert err(got[-4096:], _act64("swish", z[-4096:])) < 1e-5  # the last loop iteration's rows


class _Stores:
    """What _BN needs of an engine: parameter, gradient and statistics stores."""

    def __init__(self, device):
        from pldepth_amd.models.engine_common import FlatStore
        self.device, self.bns = device, []
        self.params, self.stats = FlatStore(), FlatStore()

    def materialize(self):
        self.params.materialize(self.device)
        self.stats.materialize(self.device)
        self.grads = self.params.like().materialize(self.device)
        for bn in self.bns:
            bn.bind(self)


@pytest.mark.parametrize("act", ["none", "relu", "swish"])
@pytest.mark.parametrize("n,hw,c", [(2, 35, 6), (3, 17, 16)])
def test_bn_add_apply_inference(cuda, n, hw, c, act):
    """_BN.add_apply(training=False): y = act(x * scale + shift + res) from the moving statistics,
    through residual_add for "none" and through bn_add_apply with identity statistics otherwise."""
    from pldepth_amd.models.engine_common import _BN
    rng = np.random.default_rng(n * hw * c)
    eng = _Stores(cuda)
    bn = _BN(eng, "bn", c)
    eng.materialize()
    gamma, beta, mmean = (rng.standard_normal(c).astype(np.float32) for _ in range(3))
    mvar = (rng.random(c) * 2).astype(np.float32)
    for t, a in ((bn.gamma, gamma), (bn.beta, beta), (bn.mmean, mmean), (bn.mvar, mvar)):
        t.copy_(torch.from_numpy(a))
    rows = n * hw
    x = rng.standard_normal((n, hw, c)).astype(np.float32)
    res = rng.standard_normal((n, hw, c)).astype(np.float32)
    tx, tres = dev(x, cuda), dev(res, cuda)
    y = torch.full_like(tx, float("nan"))
    bn.stats_(tx, rows, training=False)
    bn.add_apply(tx, rows, tres, act, y, training=False)
    torch.cuda.synchronize()
    d = np.float64
    scale = gamma.astype(d) / np.sqrt(mvar.astype(d) + d(np.float32(bn.eps)))
    shift = beta.astype(d) - mmean.astype(d) * scale
    ref = _act64(act, x.astype(d) * scale + shift + res.astype(d))
    assert err(y.cpu().numpy(), ref) < 1e-5
    assert torch.equal(tx.cpu(), torch.from_numpy(x)) and torch.equal(tres.cpu(),
                                                                      torch.from_numpy(res))
