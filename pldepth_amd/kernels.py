"""Thin Python wrappers over the C ABI, taking torch device tensors as memory handles.

PyTorch is plumbing here: tensors provide device memory and the current HIP stream; every
computation is a call into libpldepth_hip.so. Nothing here falls back to torch math.
"""
import contextlib
import ctypes as C
import os

import numpy as np

import torch

from ._lib import CONST, ConvArgs, PLDError, RefreshDesc as _RefreshDesc, lib

# selectors and limits of the C ABI, by their names in include/pldepth_hip.h
ACT = {k: CONST["PLD_ACT_" + v] for k, v in {
    "none": "NONE", "linear": "NONE", None: "NONE", "relu": "RELU", "swish": "SWISH",
    "sigmoid": "SIGMOID"}.items()}
SAMPLER = {k: CONST["PLD_SAMPLER_" + k.upper()] for k in ("pure", "masked", "thresh", "info")}


def ptr(t):
    if t is None:
        return None
    assert t.is_cuda and t.is_contiguous(), "device tensors must be contiguous HIP tensors"
    return C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _f32(t):
    assert t.dtype == torch.float32, t.dtype
    return t


_ws_cache = {}
# workspaces superseded while a captured hipGraph exists: the graph holds their raw pointers,
# so they stay allocated (never returned to the caching allocator) until every graph is gone
_ws_retired = []
_LIVE_GRAPHS = [0]


_WS_SUFFIX = [""]


@contextlib.contextmanager
def workspace_scope(suffix):
    """Every workspace requested inside the block gets its own buffer (key + suffix): calls issued
    on a second stream then never share scratch memory with the same calls on the first."""
    prev = _WS_SUFFIX[0]
    _WS_SUFFIX[0] = prev + suffix
    try:
        yield
    finally:
        _WS_SUFFIX[0] = prev


def workspace(nbytes, key="default"):
    """Reusable byte workspace on the current device (grown on demand, never shrunk)."""
    dev = torch.cuda.current_device()
    k = (dev, key + _WS_SUFFIX[0])
    buf = _ws_cache.get(k)
    if buf is None or buf.numel() < nbytes:
        if buf is not None and _LIVE_GRAPHS[0] > 0:
            _ws_retired.append(buf)
        buf = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device="cuda")
        _ws_cache[k] = buf
    return buf


# ------------------------------------------------------------------------------------- loss
def listmle_fwd_bwd(pred, y_true, B, R, L, dpred=None, nll=None, loss=None, zero_dpred=True):
    HW = pred.numel() // B
    dpred = torch.empty_like(pred) if dpred is None else dpred
    nll = torch.empty(B * R, dtype=torch.float32, device=pred.device) if nll is None else nll
    loss = torch.empty(1, dtype=torch.float32, device=pred.device) if loss is None else loss
    lib().pld_listmle_fwd_bwd(ptr(_f32(pred)), ptr(_f32(y_true)), B, HW, R, L, ptr(nll),
                              ptr(loss), ptr(dpred), int(zero_dpred), stream())
    return loss, dpred, nll


REDUCE = {"mean": CONST["PLD_REDUCE_MEAN"], "sum": CONST["PLD_REDUCE_SUM"]}


def listmle_weighted_fwd_bwd(pred, y_true, B, R, L, rank_w=None, list_w=None,
                             list_w_per_image=False, reduction="mean", dpred=None, nll=None,
                             loss=None, zero_dpred=True):
    """pld_listmle_weighted_fwd_bwd: rank_w float32 [L] (None: ones), list_w float32 [B*R], or
    [B] with list_w_per_image (None: ones), reduction "mean" | "sum". nll receives s_n nll_n."""
    HW = pred.numel() // B
    if rank_w is not None and _f32(rank_w).numel() != L:
        raise ValueError(f"rank_w holds {rank_w.numel()} weights, not L = {L}")
    if list_w is not None and _f32(list_w).numel() != (B if list_w_per_image else B * R):
        raise ValueError(f"list_w holds {list_w.numel()} weights, not "
                         f"{B if list_w_per_image else B * R}")
    dpred = torch.empty_like(pred) if dpred is None else dpred
    nll = torch.empty(B * R, dtype=torch.float32, device=pred.device) if nll is None else nll
    loss = torch.empty(1, dtype=torch.float32, device=pred.device) if loss is None else loss
    lib().pld_listmle_weighted_fwd_bwd(ptr(_f32(pred)), ptr(_f32(y_true)), B, HW, R, L,
                                       ptr(rank_w), ptr(list_w), int(bool(list_w_per_image)),
                                       REDUCE[reduction], ptr(nll), ptr(loss), ptr(dpred),
                                       int(zero_dpred), stream())
    return loss, dpred, nll


PAIRS = {"all": CONST["PLD_PAIRS_ALL"], "adjacent": CONST["PLD_PAIRS_ADJACENT"]}


def pairrank_fwd_bwd(pred, y_true, B, R, L, pair_mode="all", tau=0.03, invert=False,
                     equal_weight=1.0, list_w=None, list_w_per_image=False, reduction="mean",
                     dpred=None, per_list=None, loss=None, zero_dpred=True):
    """pld_pairrank_fwd_bwd: the pairwise ranking loss over the lists of y_true. pair_mode "all" |
    "adjacent"; tau None: the plain comparison (passed as -1.0); list_w float32 [B*R], or [B] with
    list_w_per_image (None: ones); reduction "mean" | "sum". per_list receives s_n loss_n."""
    HW = pred.numel() // B
    if pair_mode not in PAIRS:
        raise ValueError(f"unknown pair_mode {pair_mode!r} (expected one of {sorted(PAIRS)})")
    if list_w is not None and _f32(list_w).numel() != (B if list_w_per_image else B * R):
        raise ValueError(f"list_w holds {list_w.numel()} weights, not "
                         f"{B if list_w_per_image else B * R}")
    dpred = torch.empty_like(pred) if dpred is None else dpred
    per_list = torch.empty(B * R, dtype=torch.float32, device=pred.device) \
        if per_list is None else per_list
    loss = torch.empty(1, dtype=torch.float32, device=pred.device) if loss is None else loss
    lib().pld_pairrank_fwd_bwd(ptr(_f32(pred)), ptr(_f32(y_true)), B, HW, R, L, PAIRS[pair_mode],
                               -1.0 if tau is None else float(tau), int(bool(invert)),
                               float(equal_weight), ptr(list_w), int(bool(list_w_per_image)),
                               REDUCE[reduction], ptr(per_list), ptr(loss), ptr(dpred),
                               int(zero_dpred), stream())
    return loss, dpred, per_list


# ------------------------------------------------------------------------------- optimizer
def adam_amsgrad(param, grad, m, v, vhat, lr, step, beta1=0.9, beta2=0.999, eps=1e-7,
                 grad_scale=1.0):
    lib().pld_adam_amsgrad(ptr(param), ptr(grad), ptr(m), ptr(v), ptr(vhat), param.numel(),
                           float(lr), beta1, beta2, eps, int(step), float(grad_scale), stream())


def adam_amsgrad_dev(param, grad, m, v, vhat, lr_dev, step_dev, beta1=0.9, beta2=0.999,
                     eps=1e-7, grad_scale=1.0):
    lib().pld_adam_amsgrad_dev(ptr(param), ptr(grad), ptr(m), ptr(v), ptr(vhat), param.numel(),
                               ptr(lr_dev), ptr(step_dev), beta1, beta2, eps, float(grad_scale),
                               stream())


def step_increment(step_dev):
    lib().pld_step_increment(ptr(step_dev), stream())


def set_scalar(dev_tensor, value):
    lib().pld_set_scalar_f32(ptr(dev_tensor), float(value), stream())


class Graph:
    """A hipGraph captured from the current stream (pld_graph_*)."""

    def __init__(self):
        self.exec = None

    def capture(self, fn):
        self.begin()
        try:
            fn()
        except BaseException:
            self.end(failed=True)
            raise
        return self.end()

    def begin(self):
        """Start capturing the current stream (every launch until end() joins the graph)."""
        lib().pld_graph_begin(stream())
        _CAPTURING[0] = True
        # workspaces superseded during capture are retired from here on (the graph being built
        # may hold their pointers); the count stays only if the graph is instantiated
        _LIVE_GRAPHS[0] += 1
        return self

    def end(self, failed=False):
        _CAPTURING[0] = False
        h = C.c_void_p()
        try:
            lib().pld_graph_end(stream(), C.byref(h))
        except BaseException:
            _LIVE_GRAPHS[0] -= 1
            if failed:
                return self  # the capture's own exception is the one to report
            raise
        if failed:
            lib().pld_graph_destroy(h)
            _LIVE_GRAPHS[0] -= 1
            return self
        self.exec = h
        return self

    def launch(self):
        lib().pld_graph_launch(self.exec, stream())

    def __del__(self):
        if self.exec is not None:
            try:
                lib().pld_graph_destroy(self.exec)
            except Exception:
                pass
            self.exec = None
            try:
                _LIVE_GRAPHS[0] -= 1
                if _LIVE_GRAPHS[0] == 0:
                    _ws_retired.clear()
            except TypeError:  # interpreter shutdown: module globals already cleared
                pass


# ------------------------------------------------------------------------------------ conv
def same_pads(h, k, s):
    """TF 'same' padding: (pad_before, out)."""
    out = -(-h // s)
    total = max((out - 1) * s + k - h, 0)
    return total // 2, out


# conv product arithmetic (pld_conv_args.math): "bf16x3" (fp32 via three bf16 MFMA products,
# ~1e-5 relative per product) or "fp32" (exact fp32 MFMA). The model engines apply a policy
# (below); PLD_CONV_MATH overrides the default one.
MATH = {k: CONST["PLD_MATH_" + k.upper()] for k in ("fp32", "bf16x3")}
# conv arithmetic policies: "auto" (default) = decoder bf16x3, encoder bf16x3
# where the BN after the conv normalises over >= X3_MIN_POPULATION values per channel, exact
# fp32 below (BN over a handful of pixels amplifies any rounding); "mixed" = encoder fp32,
# decoder bf16x3; "bf16x3" / "fp32" everywhere
POLICIES = ("auto", "mixed", "bf16x3", "fp32")
X3_MIN_POPULATION = 4096
CONV_MATH = [os.environ.get("PLD_CONV_MATH", "auto")]


def set_conv_math(policy):
    """Default conv policy for engines built afterwards (and for conv_args() without math=)."""
    if policy not in POLICIES:
        raise ValueError(f"conv math must be one of {POLICIES}, got {policy!r}")
    CONV_MATH[0] = policy


def conv_policy(policy=None):
    """(encoder math, decoder math) of a policy (default: the current one)."""
    policy = policy or CONV_MATH[0]
    if policy not in POLICIES:
        raise ValueError(f"conv math must be one of {POLICIES}, got {policy!r}")
    if policy == "mixed":
        return ("fp32", "bf16x3")
    if policy == "auto":
        return ("auto", "bf16x3")
    return (policy, policy)


def encoder_math(enc_math, population, threshold=None):
    """Resolve an engine's encoder math for one conv whose BN sees `population` values per
    channel (batch x output pixels); `threshold` defaults to X3_MIN_POPULATION (an engine may
    carry its own: RedWebFF.x3_min_population)."""
    if enc_math != "auto":
        return enc_math
    return "bf16x3" if population >= (threshold or X3_MIN_POPULATION) else "fp32"


def conv_args(x1, x2, kh, kw, stride, pad_t, pad_l, oh, ow, cout, in_scale=None, in_shift=None,
              in_act="none", math=None):
    n, h, w, c1 = x1.shape
    c2 = 0 if x2 is None else x2.shape[3]
    a = ConvArgs()
    a.x1 = x1.data_ptr()
    a.x2 = None if x2 is None else x2.data_ptr()
    a.c1, a.c2 = c1, c2
    a.n, a.h, a.w = n, h, w
    a.kh, a.kw, a.sh, a.sw = kh, kw, stride, stride
    a.pad_t, a.pad_l = pad_t, pad_l
    a.oh, a.ow, a.cout = oh, ow, cout
    a.in_scale = None if in_scale is None else in_scale.data_ptr()
    a.in_shift = None if in_shift is None else in_shift.data_ptr()
    a.in_act = ACT[in_act]
    a.tile = -1
    a.math = MATH[math or conv_policy()[1]]
    a._keep = (x1, x2, in_scale, in_shift)  # the struct holds raw pointers: keep owners alive
    return a


def conv_kernel_name(args, mode):
    """The main kernel a conv call with these args launches (pld_conv_kernel_name)."""
    return lib().pld_conv_kernel_name(C.byref(args), {"fwd": 0, "dgrad": 1, "wgrad": 2}[mode]) \
        .decode()


def filter_to_native(w_hwio, out=None):
    kh, kw, cin, cout = w_hwio.shape
    out = torch.empty((cout, kh, kw, cin), dtype=torch.float32, device=w_hwio.device) \
        if out is None else out
    lib().pld_filter_to_native(ptr(w_hwio), kh, kw, cin, cout, ptr(out), stream())
    return out


def filter_to_dgrad(w_hwio, out=None):
    kh, kw, cin, cout = w_hwio.shape
    out = torch.empty((cin, kh, kw, cout), dtype=torch.float32, device=w_hwio.device) \
        if out is None else out
    lib().pld_filter_to_dgrad(ptr(w_hwio), kh, kw, cin, cout, ptr(out), stream())
    return out


# ---- per-shape tile autotuning (eager only; the choice never changes results) ----
AUTOTUNE = os.environ.get("PLD_AUTOTUNE", "1") != "0"
_TILE_CACHE = {}
_CAPTURING = [False]


# The persisted schedule table of the bench workloads on MI355X (written by
# `bench.py --tune`, loaded by default by bench.py and by the parity tests of the bench's
# arithmetic): with it every conv schedule of a run is fixed before the first step, no choice
# depends on timing, and the same table governs the timed run and its gradient checks.
DEFAULT_SCHEDULES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "schedules",
                                 "gfx950.json")
SCHEDULE_FORMAT = 2


def _arch():
    return torch.cuda.get_device_properties(torch.cuda.current_device()).gcnArchName \
        if torch.cuda.is_available() else "none"


def schedule_desc(math, idx):
    """Stable name of schedule `idx` (pld_conv_schedule_desc); "default" for -1 (the cost
    model's / a direct kernel's own choice)."""
    if idx < 0:
        return "default"
    d = lib().pld_conv_schedule_desc(math, idx)
    return None if d is None else d.decode()


def _schedule_index(math, desc):
    if desc == "default":
        return -1
    for i in range(lib().pld_conv_num_schedules(math)):
        if lib().pld_conv_schedule_desc(math, i).decode() == desc:
            return i
    return None


def load_tile_cache(path, arch=None):
    """Merge a schedule table written by save_tile_cache. Entries are keyed by conv shape and
    name their schedule by pld_conv_schedule_desc, so a table stays valid across library
    builds; entries whose schedule this build no longer has are dropped. Returns the number of
    entries taken (0 when the table was tuned on another GPU arch)."""
    import json
    with open(path) as f:
        d = json.load(f)
    if not isinstance(d, dict) or d.get("format") != SCHEDULE_FORMAT:
        return 0
    if d.get("arch") != (arch or _arch()):
        return 0
    taken = 0
    for k, desc in d.get("entries", []):
        k = tuple(k)
        idx = _schedule_index(k[-1], desc)
        if idx is not None:
            _TILE_CACHE[k] = idx
            taken += 1
    return taken


def save_tile_cache(path):
    import json
    entries = sorted([list(k), schedule_desc(k[-1], v)] for k, v in _TILE_CACHE.items())
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump({"format": SCHEDULE_FORMAT, "arch": _arch(),
                   "key": ["mode", "n", "h", "w", "c1", "c2", "kh", "kw", "sh", "sw", "pad_t",
                           "pad_l", "oh", "ow", "cout", "in_prologue", "math"],
                   "entries": entries}, f, indent=0)


def use_schedule_table(path=None):
    """Fix every conv schedule from a persisted table (default: DEFAULT_SCHEDULES) and turn
    timing-based tuning off: shapes the table does not hold run the cost model's choice.
    Returns (entries taken, sha1 of the file)."""
    import hashlib
    global AUTOTUNE
    path = path or DEFAULT_SCHEDULES
    with open(path, "rb") as f:
        sha = hashlib.sha1(f.read()).hexdigest()
    _TILE_CACHE.clear()
    n = load_tile_cache(path)
    AUTOTUNE = False
    return n, sha


def _shape_key(mode, a):
    return (mode, a.n, a.h, a.w, a.c1, a.c2, a.kh, a.kw, a.sh, a.sw, a.pad_t, a.pad_l, a.oh,
            a.ow, a.cout, bool(a.in_scale), a.math)


def _skinny(a):
    return (a.cout == 1 and a.kh == 3 and a.kw == 3 and a.sh == 1 and a.c2 == 0
            and not a.in_scale and a.c1 % 4 == 0 and a.c1 <= 64)


def _patch_ok(mode, a):
    """Shapes the bf16x3 patch kernels take (pld__x3_patch_ok for the FWD view of fwd / dgrad;
    pld__x3_patch_wgrad_ok for wgrad)."""
    if a.kh != 3 or a.kw != 3 or a.sh != 1 or a.sw != 1 or a.in_scale:
        return False
    if mode == "wgrad":
        return a.c1 % 16 == 0 and a.c2 % 16 == 0 and a.cout % 4 == 0
    # fwd / dgrad (FWD view: dgrad's input is dY): one 32-channel source for all three patch
    # schedules, channels in 16s per source for the multi-chunk one
    return (a.c1 % 16 == 0 and a.c2 % 16 == 0) if mode == "fwd" else a.cout % 16 == 0


def _halo_ok(mode, a):
    """Shapes the bf16x3 row-band halo kernel takes (pld__x3_halo_ok, FWD view of fwd / dgrad):
    3x3 stride 1 'same', maps up to 56 pixels wide, channels in 8s."""
    if (a.kh != 3 or a.kw != 3 or a.sh != 1 or a.sw != 1 or a.in_scale or mode == "wgrad"
            or a.oh != a.h or a.ow != a.w or a.w > 56):
        return False
    return (a.c1 % 8 == 0 and a.c2 % 8 == 0) if mode == "fwd" else a.cout % 8 == 0


def _schedules(mode, math, a=None):
    """Schedule indices worth timing (pld_conv_args.tile): fwd/dgrad every tile x split-K
    schedule (+ the patch kernel where it applies, + the tile streams); wgrad sizes its own
    split, so only the tiles (and tile streams). Under bf16x3 the exact-fp32 schedules follow
    the bf16x3 ones. A call with an input prologue cannot stream (it would run the default)."""
    n = lib().pld_conv_num_schedules(math)
    X3, PATCH, FP32, STREAM, HALO = (CONST["PLD_SCHED_" + k] for k in (
        "X3", "X3_PATCH", "FP32", "X3_STREAM", "X3_HALO"))
    out, patch_seen = [], False
    for i in range(n):
        c = lib().pld_conv_schedule_class(math, i)
        if c == PATCH and mode == "wgrad":  # one wgrad patch schedule (it sizes its own split)
            if patch_seen:
                continue
            patch_seen = True
        if mode == "wgrad" and c not in (X3, PATCH, FP32, STREAM):
            continue
        if c == STREAM and a is not None and a.in_scale:
            continue
        if c == PATCH and (a is None or not _patch_ok(mode, a)):
            continue
        if c == HALO and (a is None or not _halo_ok(mode, a)
                       or ("halo28" in schedule_desc(math, i) and a.w > 28)):
            continue
        out.append(i)
    return out


TUNE_PASSES = max(1, int(os.environ.get("PLD_TUNE_PASSES", "2")))


def _tune(mode, a, run):
    """run(tile) launches the conv into scratch outputs; returns the fastest schedule index
    (tile x split-K for fwd/dgrad; wgrad sizes its own split, so only the tile is searched)."""
    key = _shape_key(mode, a)
    if key in _TILE_CACHE:
        return _TILE_CACHE[key]
    if not AUTOTUNE or _CAPTURING[0] or _skinny(a):
        return -1
    kind = lib().pld_conv_kernel_kind(C.byref(a), {"fwd": 0, "dgrad": 1, "wgrad": 2}[mode])
    if kind == CONST["PLD_KIND_DIRECT"]:
        _TILE_CACHE[key] = -1  # direct VALU kernels (thin 1x1): no schedule to choose
        return -1
    st = torch.cuda.current_stream()
    scheds = _schedules(mode, a.math, a)
    # time in isolation: work queued on the engine's side streams (weight gradients, overlapped
    # branches) must not share the GPU with the candidates
    torch.cuda.synchronize()
    for t in scheds:
        run(t)  # warm-up (also sizes the workspace)
    # two timed passes over all candidates, best of the two per candidate: one noisy sample
    # (clock ramp, a neighbour's traffic) no longer decides the tile for the whole run
    times = {t: float("inf") for t in scheds}
    for _ in range(TUNE_PASSES):
        for t in scheds:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            run(t)
            run(t)
            e1.record(st)
            e1.synchronize()
            times[t] = min(times[t], e0.elapsed_time(e1))
    best = min(scheds, key=lambda t: times[t]) if scheds else -1
    _TILE_CACHE[key] = best
    return best


def _splitk_ws(args, fn):
    need = fn(C.byref(args))
    if need:
        ws = workspace(need, "splitk")
        args.ws, args.ws_bytes = ws.data_ptr(), ws.numel()
    else:
        args.ws, args.ws_bytes = None, 0


def filter_refresh(w_hwio, w_nat, w_nat_split=None, w_dg=None, w_dg_split=None):
    """pld_filter_refresh: native (+ split) and dgrad (+ split) filter copies of an HWIO weight in
    two passes; the split copies are attached to their fp32 tensors (as filter_split does)."""
    kh, kw, cin, cout = w_hwio.shape
    lib().pld_filter_refresh(ptr(w_hwio), kh, kw, cin, cout, ptr(w_nat), ptr(w_nat_split),
                             ptr(w_dg), ptr(w_dg_split), stream())
    if w_nat_split is not None:
        w_nat._pld_split = w_nat_split
    if w_dg_split is not None:
        w_dg._pld_split = w_dg_split


class FilterRefreshBatch:
    """Every listed filter's pld_filter_refresh in one launch (pld_filter_refresh_multi) from a
    device descriptor table built once; filters the batched path does not take (layout or
    alignment) keep their own pld_filter_refresh call. Entries: (w_hwio, w_nat, w_nat_split,
    w_dg, w_dg_split), the buffers fixed for the batch's lifetime."""

    def __init__(self, entries, device):
        self.entries = list(entries)
        descs, self.single, blk = [], [], 0
        for e in self.entries:
            w, wn, wns, wd, wds = e
            kh, kw, cin, cout = w.shape
            nb = lib().pld_filter_refresh_plan(kh, kw, cin, cout, ptr(w), ptr(wn), ptr(wns),
                                               ptr(wd), ptr(wds))
            if nb <= 0:
                self.single.append(e)
                continue
            a = [None if t is None else ptr(t).value for t in e]
            descs.append(_RefreshDesc(*a, kh * kw, cin, cout, blk, nb, 0))
            blk += nb
        self.count, self.blocks = len(descs), blk
        self.table = None
        if descs:
            arr = (_RefreshDesc * len(descs))(*descs)
            host = torch.from_numpy(np.frombuffer(bytes(arr), dtype=np.uint8).copy())
            self.table = host.to(device)
            torch.cuda.synchronize(device)
        for w, wn, wns, wd, wds in self.entries:  # the split copies ride on their fp32 tensors
            if wns is not None:
                wn._pld_split = wns
            if wds is not None:
                wd._pld_split = wds

    def __call__(self):
        if self.count:
            lib().pld_filter_refresh_multi(ptr(self.table), self.count, self.blocks, stream())
        for e in self.single:
            filter_refresh(*e)


def filter_split(w, out=None):
    """Split a [rows][K] fp32 filter (K % 8 == 0) for the bf16x3 kernel and attach the copy to
    the fp32 tensor object (w._pld_split): conv2d_fwd / conv2d_dgrad given that same tensor use
    it. The owner (engine_common._Conv.refresh) rewrites both together."""
    out = torch.empty_like(w) if out is None else out
    K_ = w.shape[-1] if w.dim() == 2 else int(np.prod(w.shape[1:]))
    rows = w.shape[0]
    lib().pld_filter_split(ptr(w), rows, K_, ptr(out), stream())
    w._pld_split = out
    return out


def _set_split(args, w):
    s = getattr(w, "_pld_split", None) if args.math == MATH["bf16x3"] else None
    args.w_split = None if s is None else s.data_ptr()


def _begin(args):
    """The caller's schedule request (-1 = tune per shape). One args object may serve the fwd,
    dgrad and wgrad of a conv: the schedule each call resolves is recorded in args._used_tile and
    args.tile is restored afterwards (_end), so a wgrad-tuned tile never leaks into the dgrad."""
    return args.tile


def _end(args, tile_in):
    args._used_tile = args.tile
    args.tile = tile_in


def _fwd_schedule(args, w_native, bias, y):
    """Resolve args.tile for a forward conv (autotuned per shape when -1) and size its split-K
    workspace."""
    if args.tile < 0:
        scratch = None

        def run(t):
            nonlocal scratch
            scratch = torch.empty_like(y) if scratch is None else scratch
            args.tile = t
            _splitk_ws(args, lib().pld_conv2d_fwd_workspace_size)
            lib().pld_conv2d_fwd(C.byref(args), ptr(w_native), ptr(bias), ptr(scratch), 0,
                                 stream())
        args.tile = _tune("fwd", args, run)
    _splitk_ws(args, lib().pld_conv2d_fwd_workspace_size)


def conv2d_fwd(args, w_native, bias, y, accumulate=False):
    tile_in = _begin(args)
    _set_split(args, w_native)
    _fwd_schedule(args, w_native, bias, y)
    lib().pld_conv2d_fwd(C.byref(args), ptr(w_native), ptr(bias), ptr(y), int(accumulate),
                         stream())
    _end(args, tile_in)
    return y


def conv2d_fwd_bn_stats(args, w_native, bias, y, mean, invstd, moving_mean=None,
                        moving_var=None, eps=1e-3, momentum=0.99):
    """conv2d_fwd + bn_stats of its output (pld_conv2d_fwd_bn_stats: the statistics gathered by
    the conv kernel's epilogue where it supports it)."""
    tile_in = _begin(args)
    _set_split(args, w_native)
    _fwd_schedule(args, w_native, bias, y)
    need = lib().pld_conv2d_fwd_bn_stats_workspace_size(C.byref(args))
    ws = workspace(need, "bnstats")
    lib().pld_conv2d_fwd_bn_stats(C.byref(args), ptr(w_native), ptr(bias), ptr(y), eps,
                                  momentum, ptr(mean), ptr(invstd), ptr(moving_mean),
                                  ptr(moving_var), ptr(ws), need, stream())
    _end(args, tile_in)
    return y


def conv2d_dgrad(args, dy, w_dgrad, dx1, dx2=None, acc1=False, acc2=False):
    tile_in = _begin(args)
    _set_split(args, w_dgrad)
    if args.tile < 0:
        s1 = s2 = None

        def run(t):
            nonlocal s1, s2
            s1 = torch.empty_like(dx1) if s1 is None else s1
            s2 = (torch.empty_like(dx2) if dx2 is not None else None) if s2 is None else s2
            args.tile = t
            _splitk_ws(args, lib().pld_conv2d_dgrad_workspace_size)
            lib().pld_conv2d_dgrad(C.byref(args), ptr(dy), ptr(w_dgrad), ptr(s1), 0, ptr(s2), 0,
                                   stream())
        args.tile = _tune("dgrad", args, run)
    _splitk_ws(args, lib().pld_conv2d_dgrad_workspace_size)
    lib().pld_conv2d_dgrad(C.byref(args), ptr(dy), ptr(w_dgrad), ptr(dx1), int(acc1), ptr(dx2),
                           int(acc2), stream())
    _end(args, tile_in)


def conv2d_wgrad(args, dy, dw, accumulate=False):
    tile_in = _begin(args)
    if args.tile < 0:
        sdw = None

        def run(t):
            nonlocal sdw
            sdw = torch.empty_like(dw) if sdw is None else sdw
            args.tile = t
            need = lib().pld_conv2d_wgrad_workspace_size(C.byref(args))
            ws = workspace(need, "wgrad") if need else None
            lib().pld_conv2d_wgrad(C.byref(args), ptr(dy), ptr(sdw), 0, ptr(ws), need, stream())
        args.tile = _tune("wgrad", args, run)
    need = lib().pld_conv2d_wgrad_workspace_size(C.byref(args))
    ws = workspace(need, "wgrad") if need else None
    lib().pld_conv2d_wgrad(C.byref(args), ptr(dy), ptr(dw), int(accumulate), ptr(ws), need,
                           stream())
    _end(args, tile_in)


def channel_sum(x, rows, c, out, accumulate=False, ws_key="reduce"):
    """out[c] (+)= sum over rows of x[rows, c]; ws_key: the workspace to use (a call on another
    stream than the BN reductions needs its own)."""
    ws = workspace(lib().pld_channel_reduce_workspace_size(rows, c), ws_key)
    lib().pld_channel_sum(ptr(x), rows, c, ptr(out), int(accumulate), ptr(ws), stream())


# -------------------------------------------------------------------------------------- BN
def bn_stats(x, rows, c, mean, invstd, moving_mean=None, moving_var=None, eps=1e-3,
             momentum=0.99):
    ws = workspace(lib().pld_channel_reduce_workspace_size(rows, c), "reduce")
    lib().pld_bn_stats(ptr(x), rows, c, eps, momentum, ptr(mean), ptr(invstd), ptr(moving_mean),
                       ptr(moving_var), ptr(ws), stream())


def bn_apply(x, rows, c, mean, invstd, gamma, beta, act, y, gate=None, hw=0):
    lib().pld_bn_apply(ptr(x), rows, c, ptr(mean), ptr(invstd), ptr(gamma), ptr(beta), ACT[act],
                       ptr(gate), hw, ptr(y), stream())


def bn_bwd(x, dy, rows, c, mean, invstd, gamma, beta, act, dx, dgamma, dbeta, gate=None,
           addn=None, hw=0, dx_accumulate=False, param_accumulate=False):
    ws = workspace(lib().pld_channel_reduce_workspace_size(rows, c), "reduce")
    lib().pld_bn_bwd(ptr(x), ptr(dy), rows, c, ptr(mean), ptr(invstd), ptr(gamma), ptr(beta),
                     ACT[act], ptr(gate), ptr(addn), hw, ptr(dx), int(dx_accumulate),
                     ptr(dgamma), ptr(dbeta), int(param_accumulate), ptr(ws), stream())


def bn_bwd_coeffs(x, dy, rows, c, mean, invstd, gamma, beta, act, dgamma, dbeta, k12,
                  param_accumulate=False):
    """pld_bn_bwd's reductions + finalize: dgamma, dbeta and k12 [2c] for pgemm_bn_bwd."""
    ws = workspace(lib().pld_channel_reduce_workspace_size(rows, c), "reduce")
    lib().pld_bn_bwd_coeffs(ptr(x), ptr(dy), rows, c, ptr(mean), ptr(invstd), ptr(gamma),
                            ptr(beta), ACT[act], ptr(dgamma), ptr(dbeta), int(param_accumulate),
                            ptr(k12), ptr(ws), stream())


def pgemm_ok(k, n):
    return bool(lib().pld_pgemm_ok(int(k), int(n)))


def pgemm_pays(k, n):
    """Where the fused pgemm beats the unfused pair (tools/pgemm_micro.py, MI355X, 448^2 batch
    32): filter K x N <= 4096 floats, i.e. it stays in the scalar cache that feeds the FMAs
    (1a/2a/2b project, 2a/2b/3a expand dgrad: 26-176 us saved each); at 144 x 40 and 240 x 40
    the filter streams from L2 per 16-wide chunk and the bf16x3 MFMA pair is faster."""
    return pgemm_ok(k, n) and k * n <= 4096


def pgemm_bn_act(x, rows, k, mean, invstd, gamma, beta, act, w, n, y, gate=None, hw=0,
                 accumulate=False):
    """y [rows, n] = (act(bn(x)) * gate[img]) . w^T  (w [n][k])."""
    lib().pld_pgemm_bn_act(ptr(x), rows, k, ptr(mean), ptr(invstd), ptr(gamma), ptr(beta),
                           ACT[act], ptr(gate), hw, ptr(w), n, ptr(y), int(accumulate), stream())


def pgemm_bn_bwd(x, dy, rows, k, mean, invstd, gamma, beta, act, k12, w, n, y,
                 accumulate=False):
    """y [rows, n] = bn_bwd(x, dy; k12) . w^T  (w [n][k])."""
    lib().pld_pgemm_bn_bwd(ptr(x), ptr(dy), rows, k, ptr(mean), ptr(invstd), ptr(gamma),
                           ptr(beta), ACT[act], ptr(k12), ptr(w), n, ptr(y), int(accumulate),
                           stream())


def pgemm_x3_ok(k, n):
    """Whether pgemm_x3_bn_act / pgemm_x3_bn_bwd take a [rows, k] x [n, k] product
    (pld_pgemm_x3_ok answers with a status)."""
    try:
        lib().pld_pgemm_x3_ok(int(k), int(n))
    except PLDError:
        return False
    return True


def pgemm_x3_pays(k, n, rows):
    """Where the fused bf16x3 pgemm (csrc/pgemm_x3.hip) is wired in place of the unfused pair
    (bn_apply + conv2d_fwd, or bn_bwd's apply + conv2d_dgrad), per shape of the 448^2 batch-32
    model: the deep-K blocks pgemm_pays leaves to the MFMA tiles. Measured with
    tools/pgemm_micro.py --family x3 on MI355X (profiles/r08_pgemm_x3_micro.txt; us per call,
    graph-replayed, median of 20, +- = largest difference between two replays; the expand
    dgrads with bn_bwd_coeffs on the fused side and the whole bn_bwd on the other):

        shape         rows    K     N    fused        pair        saved
        3a_proj      100352   144   40   34.0 +-2.6   49.6 +-3.1   15.5   wired
        3b_proj      100352   240   40   45.9 +-1.6   67.9 +-10.   22.1   wired
        4a_proj       25088   240   80   14.9 +-0.8   33.1 +-1.7   18.1   wired
        4bc_proj      25088   480   80   25.6 +-3.5   43.8 +-2.6   18.2   wired
        5a_proj       25088   480  112   28.2 +-3.3   44.2 +-3.7   15.9   wired
        5bc_proj      25088   672  112   34.3 +-3.1   52.5 +-5.7   18.2   wired
        6a_proj        6272   672  192   24.1 +-1.3   34.3 +-8.4   10.1   wired
        6bcd_proj      6272  1152  192   40.4 +-1.2   44.5 +-2.6    4.1   inside the spread
        7a_proj        6272  1152  320   59.1 +-3.2   44.8 +-7.0  -14.4   loses
        3b4a_exdg    100352   240   40   97.1 +-1.8  121.9 +-4.1   24.8   wired
        4bc5a_exdg    25088   480   80   55.9 +-1.5   73.1 +-9.6   17.1   wired
        5bc6a_exdg    25088   672  112   76.2 +-1.9   96.2 +-8.6   20.0   wired
        6bcd7a_exdg    6272  1152  192   61.4 +-1.0   61.7 +-8.6    0.3   a tie

    At 14 x 14 with K = 1152 the bf16x3 MFMA work of a 32-row strip is as long as its operand
    stream and 196 workgroups do not fill 256 CUs: those stay on the im2col tiles."""
    if not pgemm_x3_ok(k, n) or pgemm_pays(k, n):
        return False
    return (int(k), int(n), int(rows)) in PGEMM_X3_PAYS


# (K, N, rows) of the "wired" lines above (a project conv and an expand dgrad of one shape share
# a key and a verdict)
PGEMM_X3_PAYS = frozenset([(144, 40, 100352), (240, 40, 100352), (240, 80, 25088),
                           (480, 80, 25088), (480, 112, 25088), (672, 112, 25088),
                           (672, 192, 6272)])


def _split_of(w):
    s = getattr(w, "_pld_split", None)
    if s is None:
        raise PLDError("pgemm_x3: the filter has no split copy (filter_split / filter_refresh)")
    return s


def pgemm_x3_bn_act(x, rows, k, mean, invstd, gamma, beta, act, w, n, y, gate=None, hw=0,
                    accumulate=False):
    """pgemm_bn_act on bf16x3 MFMA; w [n][k] carries its pld_filter_split copy (w._pld_split)."""
    lib().pld_pgemm_x3_bn_act(ptr(x), rows, k, ptr(mean), ptr(invstd), ptr(gamma), ptr(beta),
                              ACT[act], ptr(gate), hw, ptr(_split_of(w)), n, ptr(y),
                              int(accumulate), stream())


def pgemm_x3_bn_bwd(x, dy, rows, k, mean, invstd, gamma, beta, act, k12, w, n, y,
                    accumulate=False):
    """pgemm_bn_bwd on bf16x3 MFMA; w [n][k] carries its pld_filter_split copy."""
    lib().pld_pgemm_x3_bn_bwd(ptr(x), ptr(dy), rows, k, ptr(mean), ptr(invstd), ptr(gamma),
                              ptr(beta), ACT[act], ptr(k12), ptr(_split_of(w)), n, ptr(y),
                              int(accumulate), stream())


def bn_add_apply(x, rows, c, mean, invstd, gamma, beta, res, act, y):
    lib().pld_bn_add_apply(ptr(x), rows, c, ptr(mean), ptr(invstd), ptr(gamma), ptr(beta),
                           ptr(res), ACT[act], ptr(y), stream())


def bn_scale_add_apply(x, rows, c, mean, invstd, gamma, beta, sample_scale, hw, res, act, y):
    """y = act(bn(x) * sample_scale[row // hw] + res) (pld_bn_scale_add_apply; sample_scale None:
    bn_add_apply)."""
    lib().pld_bn_scale_add_apply(ptr(x), rows, c, ptr(mean), ptr(invstd), ptr(gamma), ptr(beta),
                                 ptr(sample_scale), hw, ptr(res), ACT[act], ptr(y), stream())


def bn_bwd_scaled(x, dy, rows, c, mean, invstd, gamma, beta, act, sample_scale, hw, dx, dgamma,
                  dbeta, dx_accumulate=False, param_accumulate=False):
    """bn_bwd of dy * sample_scale[row // hw] (pld_bn_bwd_scaled)."""
    ws = workspace(lib().pld_channel_reduce_workspace_size(rows, c), "reduce")
    lib().pld_bn_bwd_scaled(ptr(x), ptr(dy), rows, c, ptr(mean), ptr(invstd), ptr(gamma),
                            ptr(beta), ACT[act], ptr(sample_scale), hw, ptr(dx),
                            int(dx_accumulate), ptr(dgamma), ptr(dbeta), int(param_accumulate),
                            ptr(ws), stream())


def bn_add_bwd(x, dy, rows, c, mean, invstd, gamma, beta, res, act, dx, dres, dgamma, dbeta,
               dx_accumulate=False, dres_accumulate=False, param_accumulate=False):
    ws = workspace(lib().pld_channel_reduce_workspace_size(rows, c), "reduce")
    lib().pld_bn_add_bwd(ptr(x), ptr(dy), rows, c, ptr(mean), ptr(invstd), ptr(gamma),
                         ptr(beta), ptr(res), ACT[act], ptr(dx), int(dx_accumulate), ptr(dres),
                         int(dres_accumulate), ptr(dgamma), ptr(dbeta), int(param_accumulate),
                         ptr(ws), stream())


def maxpool2d_fwd(x, k, s, pad_t, pad_l, y, argmax=None):
    n, h, w, c = x.shape
    oh, ow = y.shape[1], y.shape[2]
    lib().pld_maxpool2d_fwd(ptr(x), n, h, w, c, k, s, pad_t, pad_l, oh, ow, ptr(y), ptr(argmax),
                            stream())
    return y


def maxpool2d_bwd(dy, argmax, k, s, pad_t, pad_l, dx, accumulate=False):
    n, h, w, c = dx.shape
    oh, ow = dy.shape[1], dy.shape[2]
    lib().pld_maxpool2d_bwd(ptr(dy), ptr(argmax), n, h, w, c, k, s, pad_t, pad_l, oh, ow, ptr(dx),
                            int(accumulate), stream())
    return dx


def channel_affine_act(x, rows, c, scale, shift, act, y):
    lib().pld_channel_affine_act(ptr(x), rows, c, ptr(scale), ptr(shift), ACT[act], ptr(y),
                                 stream())


# ------------------------------------------------------------------------------ resampling
def upsample2x_fwd(x, y, bn=None, act="none"):
    """bn = (mean, invstd, gamma, beta): x is the pre-BN tensor; BN + act is applied to each
    tap as it is read (the activation before the upsampling is never materialised)."""
    n, h, w, c = x.shape
    if bn is None:
        lib().pld_upsample2x_fwd(ptr(x), n, h, w, c, ptr(y), stream())
    else:
        mean, invstd, gamma, beta = bn
        lib().pld_upsample2x_fwd_bn(ptr(x), n, h, w, c, ptr(mean), ptr(invstd), ptr(gamma),
                                    ptr(beta), ACT[act], ptr(y), stream())
    return y


def upsample2x_bwd(dy, dx, accumulate=False):
    n, h, w, c = dx.shape
    lib().pld_upsample2x_bwd(ptr(dy), n, h, w, c, ptr(dx), int(accumulate), stream())
    return dx


def upconv_fwd(x, bn, wt, bias, y):
    """y [n,2h,2w,1] = conv3x3(up2x(relu(bn(x)))) + bias; bn = (mean, invstd, gamma, beta)."""
    n, h, w, c = x.shape
    mean, invstd, gamma, beta = bn
    lib().pld_upconv_fwd(ptr(x), n, h, w, c, ptr(mean), ptr(invstd), ptr(gamma), ptr(beta),
                         ptr(wt), ptr(bias), ptr(y), stream())
    return y


def upconv_wgrad(x, bn, dy, dw):
    n, h, w, c = x.shape
    mean, invstd, gamma, beta = bn
    need = lib().pld_upconv_wgrad_workspace_size(c)
    ws = workspace(need, "upconv")
    lib().pld_upconv_wgrad(ptr(x), n, h, w, c, ptr(mean), ptr(invstd), ptr(gamma), ptr(beta),
                           ptr(dy), ptr(dw), ptr(ws), need, stream())


def upconv_bwd(x, bn, wt, dy, dact, dw=None, dx=None, dgamma=None, dbeta=None,
               dx_accumulate=False, param_accumulate=False):
    """The fused last stage's backward in one pass over (x, dy): dact [n,h,w,c] (gradient of
    relu(bn(x))), dw [3,3,c,1] if given, and if dx is given the BN + ReLU backward of x
    (dx, dgamma, dbeta) with its channel reductions taken in the same pass."""
    n, h, w, c = x.shape
    mean, invstd, gamma, beta = bn
    need = lib().pld_upconv_bwd_workspace_size(c)
    ws = workspace(need, "upconv")
    lib().pld_upconv_bwd(ptr(x), n, h, w, c, ptr(mean), ptr(invstd), ptr(gamma), ptr(beta),
                         ptr(wt), ptr(dy), ptr(dact), ptr(dw), ptr(dx), int(dx_accumulate),
                         ptr(dgamma), ptr(dbeta), int(param_accumulate), ptr(ws), need,
                         stream())


def upconv_dgrad(dy, wt, dact):
    """dact [n,h,w,c] = up2x^T(conv3x3^T(dy)) for dy [n,2h,2w,1], wt [3,3,c,1] (HWIO)."""
    n, h, w, c = dact.shape
    lib().pld_upconv_dgrad(ptr(dy), n, h, w, c, ptr(wt), ptr(dact), stream())


def residual_add(a, sample_scale, b, y):
    n = a.shape[0]
    lib().pld_residual_add(ptr(a), ptr(sample_scale), ptr(b), n, a.numel() // n, ptr(y),
                           stream())


def dropconnect_scales(scales, rate, seed, step, layer, image_offset=0):
    """step: an int, or a device int64 tensor (graph-replayable counter)."""
    if isinstance(step, torch.Tensor):
        lib().pld_dropconnect_scales_dev(ptr(scales), scales.numel(), float(rate), seed,
                                         ptr(step), layer, image_offset, stream())
    else:
        lib().pld_dropconnect_scales(ptr(scales), scales.numel(), float(rate), seed, step, layer,
                                     image_offset, stream())


def dropconnect_scales_multi(scales, rates, layers, seed, step, image_offset=0):
    """scales [len(layers), n]: row s = dropconnect_scales(n, rates[s], ..., layers[s]) in one
    launch; step: an int or a device int64 tensor."""
    import ctypes
    nl = len(layers)
    assert scales.dim() == 2 and scales.shape[0] == nl and scales.is_contiguous()
    assert len(rates) == nl
    dev = isinstance(step, torch.Tensor)
    # one launch per DC_MAX_LAYERS rows (the kernel's parameter block; EfficientNetB0 has 16)
    for s0 in range(0, nl, DC_MAX_LAYERS):
        m = min(DC_MAX_LAYERS, nl - s0)
        r = (ctypes.c_float * m)(*[float(x) for x in rates[s0:s0 + m]])
        l = (ctypes.c_int * m)(*[int(x) for x in layers[s0:s0 + m]])
        lib().pld_dropconnect_scales_multi(ptr(scales[s0:s0 + m]), scales.shape[1], m,
                                           ctypes.cast(r, ctypes.c_void_p),
                                           ctypes.cast(l, ctypes.c_void_p), seed,
                                           0 if dev else step, ptr(step) if dev else None,
                                           image_offset, stream())


# pld_dropconnect_scales_multi rows per launch
DC_MAX_LAYERS = CONST["PLD_DROPCONNECT_MAX_LAYERS"]


def bn_train_coeffs(mean, invstd, gamma, beta, scale, shift):
    """Training-mode BN as act-free affine coefficients (scale = gamma*invstd, shift = beta -
    mean*scale): the consuming conv's input prologue (conv_args in_scale / in_shift)."""
    lib().pld_bn_train_coeffs(ptr(mean), ptr(invstd), ptr(gamma), ptr(beta), gamma.numel(),
                              ptr(scale), ptr(shift), stream())


def channel_pad_affine(x, cout, y, scale=None, shift=None):
    """y [.., cout] = [x*scale + shift | 0] of x [.., cin] (the stem's widened input)."""
    cin = x.shape[-1]
    lib().pld_channel_pad_affine(ptr(x), x.numel() // cin, cin, cout, ptr(scale), ptr(shift),
                                 ptr(y), stream())
    return y


def bn_inference_coeffs(gamma, beta, mmean, mvar, scale, shift, eps=1e-3):
    lib().pld_bn_inference_coeffs(ptr(gamma), ptr(beta), ptr(mmean), ptr(mvar), gamma.numel(),
                                  eps, ptr(scale), ptr(shift), stream())


def scale_per_sample(x, sample_scale, y, accumulate=False):
    n = x.shape[0]
    lib().pld_scale_per_sample(ptr(x), ptr(sample_scale), n, x.numel() // n, ptr(y),
                               int(accumulate), stream())


# ------------------------------------------------------------------------- depthwise / SE
def dwconv_fwd(x, wdw, k, s, pad_t, pad_l, y, bn=None, act="none"):
    """bn = (mean, invstd, gamma, beta): x is the producer's pre-BN tensor and the training-mode
    BN + act is applied as the pixels are read (no materialised activation)."""
    n, h, w, c = x.shape
    _, oh, ow, _ = y.shape
    if bn is None:
        lib().pld_dwconv_fwd(ptr(x), n, h, w, c, ptr(wdw), k, s, pad_t, pad_l, oh, ow, ptr(y),
                             stream())
    else:
        mean, invstd, gamma, beta = bn
        lib().pld_dwconv_fwd_bn(ptr(x), n, h, w, c, ptr(wdw), k, s, pad_t, pad_l, oh, ow,
                                ptr(mean), ptr(invstd), ptr(gamma), ptr(beta), ACT[act], ptr(y),
                                stream())


def dwconv_fwd_bn_stats(x, wdw, k, s, pad_t, pad_l, y, ybn, bn=None, act="none", eps=1e-3,
                        momentum=0.99):
    """dwconv_fwd + the batch statistics of y for the BN after it: ybn = (mean, invstd,
    moving_mean, moving_var) written like bn_stats (gathered in the tiled kernel's epilogue)."""
    n, h, w, c = x.shape
    _, oh, ow, _ = y.shape
    need = lib().pld_dwconv_fwd_bn_stats_workspace_size(n, oh, ow, c, s)
    ws = workspace(need, "bnstats")
    mean, invstd, gamma, beta = bn if bn is not None else (None,) * 4
    ym, yi, ymm, ymv = ybn
    lib().pld_dwconv_fwd_bn_stats(ptr(x), n, h, w, c, ptr(wdw), k, s, pad_t, pad_l, oh, ow,
                                  ptr(mean), ptr(invstd), ptr(gamma), ptr(beta), ACT[act],
                                  ptr(y), eps, momentum, ptr(ym), ptr(yi), ptr(ymm), ptr(ymv),
                                  ptr(ws), need, stream())


def dwconv_dgrad(dy, wdw, k, s, pad_t, pad_l, dx, accumulate=False):
    n, h, w, c = dx.shape
    _, oh, ow, _ = dy.shape
    lib().pld_dwconv_dgrad(ptr(dy), n, h, w, c, ptr(wdw), k, s, pad_t, pad_l, oh, ow, ptr(dx),
                           int(accumulate), stream())


def dwconv_dgrad_bn_bwd(dy, wdw, k, s, pad_t, pad_l, dact, x, bn, act, dgamma, dbeta, k12,
                        dx=None, accumulate=False, dx_accumulate=False, param_accumulate=False):
    """dwconv_dgrad into dact with the backward of the BN + act that produced the depthwise input
    (x: that BN's input; bn = (mean, invstd, gamma, beta)) fused: its reductions in the dgrad's
    epilogue, then dgamma/dbeta/k12, and dx (the BN input gradient) when given."""
    n, h, w, c = dact.shape
    _, oh, ow, _ = dy.shape
    need = lib().pld_dwconv_dgrad_bn_bwd_workspace_size(n, h, w, c, s)
    ws = workspace(need, "dwbnb")
    mean, invstd, gamma, beta = bn
    lib().pld_dwconv_dgrad_bn_bwd(ptr(dy), n, h, w, c, ptr(wdw), k, s, pad_t, pad_l, oh, ow,
                                  ptr(dact), int(accumulate), ptr(x), ptr(mean), ptr(invstd),
                                  ptr(gamma), ptr(beta), ACT[act], ptr(dx), int(dx_accumulate),
                                  ptr(dgamma), ptr(dbeta), int(param_accumulate), ptr(k12),
                                  ptr(ws), need, stream())


def dwconv_dgrad_se_bn(dy, x, bn, k12, gate, addn, wdw, k, pad_t, pad_l, dact, ex=None, ebn=None,
                       edgamma=None, edbeta=None, ek12=None, edx=None, act="swish", eact="swish",
                       accumulate=False, param_accumulate=False):
    """The stride-1 dwconv_dgrad of an MBConv block read straight from the SE output's gradient
    dy: the block BN's backward (x: its input, bn = (mean, invstd, gamma, beta), k12 / addn from
    se_bwd_bn_coeffs, the SE gate) is applied as the window is staged, so the dx of
    se_bwd_bn_full is never written. With ex / ebn (the expand BN and its input) the dgrad's
    epilogue also gathers that BN's backward sums: edgamma, edbeta and ek12 as bn_bwd_coeffs
    leaves them, and edx (when given) that BN's input gradient. Raises PLDError where the LDS-tiled kernel does not take the layer."""
    n, h, w, c = dact.shape
    _, oh, ow, _ = dy.shape
    mean, invstd, gamma, beta = bn
    em, ei, eg, eb = ebn if ex is not None else (None,) * 4
    need = lib().pld_dwconv_dgrad_se_bn_workspace_size(n, h, w, c) if ex is not None else 0
    ws = workspace(need, "dwbnb") if need else None
    lib().pld_dwconv_dgrad_se_bn(ptr(dy), ptr(x), n, h, w, c, ptr(wdw), k, pad_t, pad_l, oh, ow,
                                 ptr(mean), ptr(invstd), ptr(gamma), ptr(beta), ptr(k12), ACT[act],
                                 ptr(gate), ptr(addn), ptr(dact), int(accumulate), ptr(ex),
                                 ptr(em), ptr(ei), ptr(eg), ptr(eb), ACT[eact], ptr(edgamma),
                                 ptr(edbeta), int(param_accumulate), ptr(ek12), ptr(edx), ptr(ws),
                                 need, stream())


def dw_dgrad_fuse_ok(k, c):
    """The layers dwconv_dgrad_se_bn / the tiled dwconv_dgrad_bn_bwd take (stride 1)."""
    return k in (3, 5) and c % 16 == 0


def dw_dgrad_fuse_pays(k, c, h):
    """(pro, epi): the stages EffNetFF wires into the stride-1 depthwise dgrad of a block with
    a k x k filter, c expanded channels and an h x h map: the block BN's backward applied on
    load (pro), the expand BN's backward sums gathered on store (epi).

    Measured (tools/dw_fuse_micro.py, MI355X, 448^2 batch 32, graph replays, median us of SE
    backward + dgrad + expand BN reductions, spread <= 5 us; profiles/r07_dw_fuse_micro.txt):

        blocks    shape            pair    pro    epi   both
        1a        224^2 x 32  k3  278.9  219.9      -      -
        2b        112^2 x 144 k3  413.9  376.8  386.3  345.1
        3b        56^2 x 240  k5  203.0  185.3  185.2  163.7
        4b 4c     28^2 x 480  k3  112.4   96.1   97.9   87.3
        5a        28^2 x 480  k5  124.8  110.4  109.2   99.3
        5b 5c     28^2 x 672  k5  168.0  152.7  147.9  133.4
        6b 6c 6d  14^2 x 1152 k5   95.8   87.2   88.1   80.5
        7a        14^2 x 1152 k3   87.9   79.3   81.2   73.6

    Both stages pay at every shape, so pro is wired everywhere. epi is not: its sums reach k12 in
    another (fixed) order, 1e-8 away, and the 15 project-BN beta gradients, which are zero
    analytically (a shift in front of a training-mode BN) and rounding residue of 1e-5 .. 1e-3
    beside gradients of 1e3 in practice, then move by their own size; the engine's gradients
    stay bit for bit what the unfused pair gives. PLD_DW_SE_BN=both wires it (step 15.09 ->
    14.80 ms against 14.91 ms with pro alone, profiles/r07_dw_fuse_step_ab.txt)."""
    return True, False


def se_fwd(a, w1, b1, w2, b2, pooled, z1, gate, bn=None, act="swish"):
    """bn = (mean, invstd, gamma, beta): `a` is the pre-BN tensor; the squeeze applies BN + act."""
    n, h, w, c = a.shape
    cse = w1.shape[-1]
    ws = workspace(lib().pld_se_workspace_size(n, h * w, c, cse), "se")
    if bn is None:
        lib().pld_se_fwd(ptr(a), n, h * w, c, cse, ptr(w1), ptr(b1), ptr(w2), ptr(b2),
                         ptr(pooled), ptr(z1), ptr(gate), ptr(ws), stream())
    else:
        mu, inv, g, b = bn
        lib().pld_se_fwd_bn(ptr(a), ptr(mu), ptr(inv), ptr(g), ptr(b), ACT[act], n, h * w, c,
                            cse, ptr(w1), ptr(b1), ptr(w2), ptr(b2), ptr(pooled), ptr(z1),
                            ptr(gate), ptr(ws), stream())


def se_bwd(dy, a, w1, w2, z1, gate, addn, bn=None, act="swish"):
    n, h, w, c = a.shape
    cse = w1.shape[-1]
    ws = workspace(lib().pld_se_workspace_size(n, h * w, c, cse), "se")
    if bn is None:
        lib().pld_se_bwd(ptr(dy), ptr(a), n, h * w, c, cse, ptr(w1), ptr(w2), ptr(z1),
                         ptr(gate), ptr(addn), ptr(ws), stream())
    else:
        mu, inv, g, b = bn
        lib().pld_se_bwd_bn(ptr(dy), ptr(a), ptr(mu), ptr(inv), ptr(g), ptr(b), ACT[act], n,
                            h * w, c, cse, ptr(w1), ptr(w2), ptr(z1), ptr(gate), ptr(addn),
                            ptr(ws), stream())


def se_bwd_bn_full(dy, x, bn, w1, w2, z1, gate, addn, dx, dgamma, dbeta, act="swish",
                   dx_accumulate=False, param_accumulate=False):
    """SE backward (addn) + the block BN's backward (dx, dgamma, dbeta) with the BN reductions
    gathered by the SE squeeze sweep over (x, dy): pld_se_bwd_bn_full."""
    n, h, w, c = x.shape
    cse = w1.shape[-1]
    need = lib().pld_se_bwd_bn_full_workspace_size(n, h * w, c, cse)
    ws = workspace(need, "se_bn")
    mu, inv, g, b = bn
    lib().pld_se_bwd_bn_full(ptr(dy), ptr(x), ptr(mu), ptr(inv), ptr(g), ptr(b), ACT[act], n,
                             h * w, c, cse, ptr(w1), ptr(w2), ptr(z1), ptr(gate), ptr(addn),
                             ptr(dx), int(dx_accumulate), ptr(dgamma), ptr(dbeta),
                             int(param_accumulate), ptr(ws), need, stream())


def se_bwd_bn_coeffs(dy, x, bn, w1, w2, z1, gate, addn, dgamma, dbeta, k12, act="swish",
                     param_accumulate=False):
    """se_bwd_bn_full without its elementwise pass: addn, dgamma, dbeta and the block BN's
    k12 [2c] for dwconv_dgrad_se_bn, which applies the backward as it reads (no dx)."""
    n, h, w, c = x.shape
    cse = w1.shape[-1]
    need = lib().pld_se_bwd_bn_full_workspace_size(n, h * w, c, cse)
    ws = workspace(need, "se_bn")
    mu, inv, g, b = bn
    lib().pld_se_bwd_bn_coeffs(ptr(dy), ptr(x), ptr(mu), ptr(inv), ptr(g), ptr(b), ACT[act], n,
                               h * w, c, cse, ptr(w1), ptr(w2), ptr(z1), ptr(gate), ptr(addn),
                               ptr(dgamma), ptr(dbeta), int(param_accumulate), ptr(k12), ptr(ws),
                               need, stream())


# -------------------------------------------------------------------------------- sampler
def sampler_candidates(R, strategy):
    return lib().pld_sampler_candidates(R, SAMPLER[strategy])


def sampler_compact(mask, gt, valid_idx, nvalid, gt_minmax):
    B, H, W = mask.shape
    ws = workspace(lib().pld_sampler_compact_workspace_size(B, H, W), "compact")
    lib().pld_sampler_compact(ptr(mask), B, H, W, ptr(gt), ptr(valid_idx), ptr(nvalid),
                              ptr(gt_minmax), ptr(ws), stream())


def sampler_draw(nvalid, n_cand, L, seed, step, image_offset, draws):
    """step: an int, or a device int64 tensor (graph-replayable counter)."""
    B = nvalid.shape[0]
    if isinstance(step, torch.Tensor):
        lib().pld_sampler_draw_dev(ptr(nvalid), B, n_cand, L, seed, ptr(step), image_offset,
                                   ptr(draws), stream())
    else:
        lib().pld_sampler_draw(ptr(nvalid), B, n_cand, L, seed, step, image_offset, ptr(draws),
                               stream())


def sampler_rank(gt, valid_idx, nvalid, gt_minmax, draws, R, L, strategy, out):
    B, H, W = gt.shape
    sid = SAMPLER[strategy]
    ws = workspace(lib().pld_sampler_workspace_size(B, H, W, R, L, sid), "sampler")
    lib().pld_sampler_rank(ptr(gt), ptr(valid_idx), ptr(nvalid), ptr(gt_minmax), ptr(draws), B,
                           H, W, R, L, sid, ptr(out), ptr(ws), stream())
    return out


# pld_sampler_rank_ex also takes the unmasked RandomSamplingStrategy
SAMPLER_EX = dict(SAMPLER, random=CONST["PLD_SAMPLER_RANDOM"])


def sampler_rank_ex_workspace_size(B, n_cand, L):
    need = C.c_size_t()
    lib().pld_sampler_rank_ex_workspace_size(B, n_cand, L, C.byref(need))
    return need.value


def sampler_rank_ex(gt, valid_idx, nvalid, gt_minmax, draws, R, L, strategy, out, n_cand,
                    tau=0.03, penalty=-1000, mask_shape=None):
    """sampler_rank with the strategy classes' arguments: n_cand = int(R * batch_size_factor),
    tau, penalty and the mask's grid (mask_shape (h, w); None: the image's). valid_idx / nvalid
    index the mask grid; both are None for the unmasked "random" strategy."""
    B, H, W = gt.shape
    mh, mw = (H, W) if mask_shape is None else mask_shape
    need = sampler_rank_ex_workspace_size(B, n_cand, L)
    ws = workspace(need, "sampler_ex")
    lib().pld_sampler_rank_ex(ptr(gt), ptr(valid_idx), ptr(nvalid), ptr(gt_minmax), ptr(draws),
                              B, H, W, mh, mw, R, L, n_cand, SAMPLER_EX[strategy], float(tau),
                              float(penalty), ptr(out), ptr(ws), need, stream())
    return out


def sampler_minmax(gt, gt_minmax):
    """gt [B,H,W] -> gt_minmax [B,2]: np.amin / np.amax per image (the Info strategy's bounds when
    the mask is on another grid and sampler_compact cannot give them)."""
    B, H, W = gt.shape
    lib().pld_sampler_minmax(ptr(gt), B, H, W, ptr(gt_minmax), stream())


# ---- test-pass metrics (pld_ordinal_error / pld_dcg_ratio) ----
def ordinal_error(pred, gt, idx0, idx1):
    """pred, gt: [n, hw] float32 device tensors; idx0/idx1: int32 device indices -> [n] float64."""
    n, hw = pred.shape[0], pred[0].numel()
    assert gt.shape[0] == n and gt[0].numel() == hw and idx0.numel() == idx1.numel()
    assert idx0.dtype == torch.int32 and idx1.dtype == torch.int32
    out = torch.empty(n, dtype=torch.float64, device=pred.device)
    lib().pld_ordinal_error(ptr(_f32(pred)), ptr(_f32(gt)), n, hw, ptr(idx0), ptr(idx1),
                            idx0.numel(), ptr(out), stream())
    return out


def dcg_ratio(pred, gt, ids):
    """pred, gt: [n, hw] float32 device tensors; ids: int32 device list -> [n] float64."""
    n, hw = pred.shape[0], pred[0].numel()
    assert gt.shape[0] == n and gt[0].numel() == hw and ids.dtype == torch.int32
    out = torch.empty(n, dtype=torch.float64, device=pred.device)
    lib().pld_dcg_ratio(ptr(_f32(pred)), ptr(_f32(gt)), n, hw, ptr(ids), ids.numel(), ptr(out),
                        stream())
    return out


# ---- depth-edge metrics (pld_minmax_u8 / pld_*canny_u8 / pld_chamfer_dt3 / pld_depth_edge_metric)
EDGE_MAX_DIM = CONST["PLD_EDGE_MAX_DIM"]  # largest map side the Canny entry points take


def _u8_maps(t):
    assert t.dtype == torch.uint8 and t.dim() == 3, (t.dtype, tuple(t.shape))
    return t.shape


def minmax_u8(x):
    """x: [n, ...] float32 device tensor -> uint8 tensor of the same shape, each image min-max
    scaled to 0..255 (cv2.normalize NORM_MINMAX + astype(uint8))."""
    n, hw = x.shape[0], x[0].numel()
    out = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    ws = workspace(lib().pld_minmax_u8_workspace_size(n), "minmax_u8")
    lib().pld_minmax_u8(ptr(_f32(x)), n, hw, ptr(out), ptr(ws), stream())
    return out


def canny(img, lo, hi, sweeps=None):
    """img: [n, h, w] uint8 device tensor -> [n, h, w] uint8 edge maps (0 / 255) of
    cv2.Canny(img, lo, hi). sweeps: optional [n] int32 device tensor, receives the number of
    hysteresis passes per image."""
    n, h, w = _u8_maps(img)
    out = torch.empty_like(img)
    ws = workspace(lib().pld_canny_workspace_size(n, h, w), "canny")
    lib().pld_canny_u8(ptr(img), n, h, w, int(lo), int(hi), ptr(out), ptr(sweeps), ptr(ws),
                       stream())
    return out


def auto_canny(img, sigma=1.8, sweeps=None):
    """img: [n, h, w] uint8 device tensor -> (edges [n, h, w] uint8, thresholds [n, 2] int32) of
    the reference's auto_canny(img, sigma): Canny between int(max(0, (1 - sigma) * median)) and
    int(min(255, (1 + sigma) * median)), per image."""
    n, h, w = _u8_maps(img)
    out = torch.empty_like(img)
    thr = torch.empty((n, 2), dtype=torch.int32, device=img.device)
    ws = workspace(lib().pld_canny_workspace_size(n, h, w), "canny")
    lib().pld_auto_canny_u8(ptr(img), n, h, w, 1.0 - sigma, 1.0 + sigma, ptr(thr), ptr(out),
                            ptr(sweeps), ptr(ws), stream())
    return out, thr


def chamfer_dt3(mask, max_dist=10.0):
    """mask: [n, h, w] uint8 device tensor -> [n, h, w] float32: at non-zero pixels the 3x3
    chamfer distance to the nearest zero pixel (cv2.distanceTransform DIST_L2, 3), 0 where it
    exceeds max_dist; 0 at zero pixels."""
    n, h, w = _u8_maps(mask)
    out = torch.empty(mask.shape, dtype=torch.float32, device=mask.device)
    lib().pld_chamfer_dt3(ptr(mask), n, h, w, float(max_dist), ptr(out), stream())
    return out


def depth_edge_metric(edges_op, edges_gt):
    """edges_op, edges_gt: [n, h, w] uint8 edge maps -> [n, 2] float64
    (depth_boundary_error, completeness_error) per image."""
    n, h, w = _u8_maps(edges_op)
    assert tuple(edges_gt.shape) == (n, h, w) and edges_gt.dtype == torch.uint8
    out = torch.empty((n, 2), dtype=torch.float64, device=edges_op.device)
    lib().pld_depth_edge_metric(ptr(edges_op), ptr(edges_gt), n, h, w, ptr(out), stream())
    return out


# ---- active-learning selection (active.hip) ----
MEDIAN_MAX_KSIZE = CONST["PLD_MEDIAN_MAX_KSIZE"]
TILE_MAX = CONST["PLD_TILE_MAX"]  # largest tile side of the tile entry points
ORACLE_MAX_L = CONST["PLD_ORACLE_MAX_L"]


def gray(rgb):
    """rgb: [n, h, w, 3] float32 device tensor -> [n, h, w] float32 (cv2 RGB2GRAY)."""
    assert rgb.dim() == 4 and rgb.shape[-1] == 3, tuple(rgb.shape)
    n, h, w, _ = rgb.shape
    out = torch.empty((n, h, w), dtype=torch.float32, device=rgb.device)
    lib().pld_gray_f32(ptr(_f32(rgb)), n, h * w, ptr(out), stream())
    return out


def median_blur(img, ksize):
    """img: [n, h, w] uint8 device tensor -> cv2.medianBlur(img, ksize) per image."""
    n, h, w = _u8_maps(img)
    out = torch.empty_like(img)
    lib().pld_median_blur_u8(ptr(img), n, h, w, int(ksize), ptr(out), stream())
    return out


def unsharp(x, sigma=1.0, amount=3.0, normalize=True):
    """x: [n, h, w] float32 device tensor -> [n, h, w] uint8: each map min-max scaled to 0..255
    as float32 (normalize=False: taken as it is) and sharpened by the reference's
    unsharp_mask((5, 5), sigma, amount)."""
    assert x.dim() == 3, tuple(x.shape)
    n, h, w = x.shape
    out = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    ws = workspace(lib().pld_unsharp_u8_workspace_size(n), "unsharp_u8")
    lib().pld_unsharp_u8(ptr(_f32(x)), n, h, w, int(bool(normalize)), float(sigma), float(amount),
                         ptr(out), ptr(ws), stream())
    return out


def tile_hausdorff(edges_in, edges_pred, split):
    """edges_in, edges_pred: [n, h, h] uint8 edge maps -> [n, split^2, 8] int32 per tile:
    (hd2, in_r, in_c, pred_r, pred_c, n_in, n_pred, branch), see pld_tile_hausdorff."""
    n, h, w = _u8_maps(edges_in)
    assert tuple(edges_pred.shape) == (n, h, w) and edges_pred.dtype == torch.uint8
    out = torch.empty((n, split * split, 8), dtype=torch.int32, device=edges_in.device)
    lib().pld_tile_hausdorff(ptr(edges_in), ptr(edges_pred), n, h, w, int(split), ptr(out),
                             stream())
    return out


def tile_nth_edge(edges_in, split, k, rc):
    """For tiles with k[image, tile] >= 0, rc[image, tile] = tile-local (r, c) of the tile's k-th
    non-zero pixel; other entries of rc (int32 [n, split^2, 2]) stay as they are."""
    n, h, w = _u8_maps(edges_in)
    assert k.dtype == torch.int32 and tuple(k.shape) == (n, split * split)
    assert rc.dtype == torch.int32 and tuple(rc.shape) == (n, split * split, 2)
    lib().pld_tile_nth_edge(ptr(edges_in), n, h, w, int(split), ptr(k), ptr(rc), stream())
    return rc


def al_oracle(gt, pos_xy, L, row_stride):
    """gt: [n, h, w] float32, pos_xy: [n, P, 2] int32 (r, c) -> [n, P // L, L, 2] float32
    rankings (flat index r * row_stride + c, depth), see pld_al_oracle."""
    n, h, w = gt.shape
    assert pos_xy.dtype == torch.int32 and pos_xy.dim() == 3 and pos_xy.shape[0] == n
    P = pos_xy.shape[1]
    out = torch.empty((n, P // L, L, 2), dtype=torch.float32, device=gt.device)
    if out.numel() == 0:  # fewer points than one ranking
        return out
    lib().pld_al_oracle(ptr(_f32(gt)), n, h, w, ptr(pos_xy), P, int(L), int(row_stride), ptr(out),
                        stream())
    return out


# ---- test-set evaluation (evalset.hip) ----
RANKING_MAX_L = CONST["PLD_RANKING_MAX_L"]
MAX_INDEXED_PIXELS = 1 << 24  # flat pixel indices are carried as float32


def _check_pixels(who, hw):
    if hw > MAX_INDEXED_PIXELS:
        raise ValueError(f"{who}: {hw} pixels per image; flat indices are stored as float32, "
                         f"exact up to {MAX_INDEXED_PIXELS}")


def ordinal_pairs(gt, coords, tau=0.03, invert=False):
    """gt: [n, h, w] float32 device tensor; coords: host integers [n, P, 4] = (x0, y0, x1, y1),
    x the row -> [n, P, 5] float32 device table (p0, p1, relation, z0, z1), see
    pld_ordinal_pairs. tau=None: the plain comparison."""
    n, h, w = gt.shape
    _check_pixels("ordinal_pairs", h * w)
    coords = np.asarray(coords)  # drawn on the host, and checked there before any launch
    if coords.dtype.kind not in "iu" or coords.size == 0 or coords.ndim != 3 \
            or coords.shape[0] != n or coords.shape[2] != 4:
        raise ValueError(f"ordinal_pairs: expected non-empty integers [{n}, P, 4], got "
                         f"{coords.dtype} {coords.shape}")
    lim = np.array([h, w, h, w])
    if coords.min() < 0 or (coords >= lim).any():
        bad = coords[((coords < 0) | (coords >= lim)).any(-1)][0]
        raise ValueError(f"ordinal_pairs: point {tuple(int(v) for v in bad)} outside a map of "
                         f"{h} x {w} pixels")
    P = coords.shape[1]
    c = torch.from_numpy(np.ascontiguousarray(coords, np.int32)).to(gt.device)
    out = torch.empty((n, P, 5), dtype=torch.float32, device=gt.device)
    lib().pld_ordinal_pairs(ptr(_f32(gt)), n, h, w, ptr(c), P,
                            -1.0 if tau is None else float(tau), int(bool(invert)), ptr(out),
                            stream())
    return out


def depth_rankings(gt, idx, invert=False):
    """gt: [n, h, w] or [n, hw] float32 device tensor; idx: host integers [n, R, L] flat pixel
    indices -> [n, R, L, 2] float32 device rankings (index, depth), see pld_depth_rankings."""
    n, hw = gt.shape[0], gt[0].numel()
    _check_pixels("depth_rankings", hw)
    idx = np.asarray(idx)
    if idx.dtype.kind not in "iu" or idx.ndim != 3 or idx.size == 0 or idx.shape[0] != n:
        raise ValueError(f"depth_rankings: expected non-empty integers [{n}, R, L], got "
                         f"{idx.dtype} {idx.shape}")
    if idx.min() < 0 or idx.max() >= hw:
        bad = int(idx.min() if idx.min() < 0 else idx.max())
        raise ValueError(f"depth_rankings: index {bad} outside an image of {hw} pixels")
    _, R, L = idx.shape
    d = torch.from_numpy(np.ascontiguousarray(idx, np.int32)).to(gt.device)
    out = torch.empty((n, R, L, 2), dtype=torch.float32, device=gt.device)
    lib().pld_depth_rankings(ptr(_f32(gt)), n, hw, ptr(d), R, L, int(bool(invert)), ptr(out),
                             stream())
    return out


def ordinal_pair_error(pred, pairs, tau=None, invert=False):
    """pred: [n, ...] float32 device predictions of hw pixels each; pairs: [n, P, 5] float32
    device table of ordinal_pairs -> (wrong [n], counted [n]) int32 device tensors, see
    pld_ordinal_pair_error. tau=None: the table's relations; else they are recomputed from its
    depths at tau and invert."""
    n, hw = pred.shape[0], pred[0].numel()
    _check_pixels("ordinal_pair_error", hw)
    assert pairs.dim() == 3 and pairs.shape[0] == n and pairs.shape[2] == 5, tuple(pairs.shape)
    wrong = torch.empty(n, dtype=torch.int32, device=pred.device)
    counted = torch.empty(n, dtype=torch.int32, device=pred.device)
    lib().pld_ordinal_pair_error(ptr(_f32(pred)), n, hw, ptr(_f32(pairs)), pairs.shape[1],
                                 0.0 if tau is None else float(tau), int(tau is not None),
                                 int(bool(invert)), ptr(wrong), ptr(counted), stream())
    return wrong, counted


def antialias_taps(n_in, n_out):
    """The centre and one side of the normalised Gaussian skimage.transform.resize blurs an axis
    with before it shrinks it from n_in to n_out (float64): sigma = max(0, (n_in / n_out - 1) /
    2), radius int(4 sigma + 0.5), weights exp(-0.5 / sigma^2 * d^2) / sum as
    scipy.ndimage.gaussian_filter forms them. [1.] when nothing is blurred."""
    sigma = max(0.0, (n_in / n_out - 1) / 2)
    radius = int(4.0 * sigma + 0.5)
    if sigma <= 0 or radius == 0:
        return np.ones(1)
    d = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * d ** 2)
    phi = phi / phi.sum()
    return np.ascontiguousarray(phi[radius:])


def resize_antialias(x, oh, ow, out=None):
    """x: [n, h, w, c] float32 device tensor -> [n, oh, ow, c]: skimage.transform.resize(order 1,
    mode 'reflect', anti-aliasing when shrinking), see pld_resize_antialias."""
    n, h, w, c = x.shape
    out = torch.empty((n, oh, ow, c), dtype=torch.float32, device=x.device) if out is None else out
    wy, wx = antialias_taps(h, oh), antialias_taps(w, ow)
    taps = torch.from_numpy(np.concatenate([wy, wx])).to(x.device)  # one upload
    lib().pld_resize_antialias(ptr(_f32(x.contiguous())), n, h, w, c, oh, ow, ptr(taps[:len(wy)]),
                               len(wy) - 1, ptr(taps[len(wy):]), len(wx) - 1, ptr(out), stream())
    return out


# ---- HR-WSI resizing (pld_resize_bilinear / pld_resize_nearest) ----
def resize(x, oh, ow, method="bilinear", out=None):
    """x: [n, h, w, c] float32 device tensor -> [n, oh, ow, c] (tf.image.resize, TF2 semantics)."""
    n, h, w, c = x.shape
    out = torch.empty((n, oh, ow, c), dtype=torch.float32, device=x.device) if out is None else out
    fn = lib().pld_resize_bilinear if method == "bilinear" else lib().pld_resize_nearest
    fn(ptr(_f32(x.contiguous())), n, h, w, c, oh, ow, ptr(out), stream())
    return out


# ---- device-resident training batches (pld_batch_gather_flip) ----
def batch_gather_flip(imgs, gts, masks, idx, flip, out=None):
    """imgs [n, h, w, c], gts / masks [n, h, w] (or None) float32 device tensors; idx: B host
    integers in [0, n); flip: B host 0/1 values or None -> (x [B, h, w, c], gt, mask [B, h, w]):
    x[b] = imgs[idx[b]], mirrored left-right where flip[b] (gt and mask with it; None where the
    source is None). ``out``: the (x, gt, mask) tensors to fill instead of fresh ones."""
    n, h, w, c = imgs.shape
    idx = np.asarray(idx)
    if idx.ndim != 1 or idx.size == 0 or idx.dtype.kind not in "iu":
        raise ValueError(f"batch_gather_flip: idx must be a non-empty 1-d integer array, "
                         f"got {idx.dtype} {idx.shape}")
    if idx.min() < 0 or idx.max() >= n:  # the kernel does not check: see pld_batch_gather_flip
        bad = int(idx.min() if idx.min() < 0 else idx.max())
        raise ValueError(f"batch_gather_flip: index {bad} outside a dataset of {n} images")
    B = idx.size
    sel = np.zeros((2, B), np.int32)  # one upload: indices, then flips
    sel[0] = idx
    if flip is not None:
        flip = np.asarray(flip)
        if flip.shape != (B,):
            raise ValueError(f"batch_gather_flip: flip has shape {flip.shape}, idx {idx.shape}")
        sel[1] = flip != 0
    for t in (gts, masks):
        assert t is None or tuple(t.shape) == (n, h, w), (tuple(t.shape), (n, h, w))
    dev = imgs.device
    if out is None:
        x = torch.empty((B, h, w, c), dtype=torch.float32, device=dev)
        gt = None if gts is None else torch.empty((B, h, w), dtype=torch.float32, device=dev)
        mask = None if masks is None else torch.empty((B, h, w), dtype=torch.float32, device=dev)
    else:
        x, gt, mask = out
        assert tuple(x.shape) == (B, h, w, c) and (gt is None) == (gts is None) \
            and (mask is None) == (masks is None)
        assert all(t is None or tuple(t.shape) == (B, h, w) for t in (gt, mask))
    sel_d = torch.from_numpy(sel).to(dev)
    lib().pld_batch_gather_flip(
        ptr(_f32(imgs)), ptr(None if gts is None else _f32(gts)),
        ptr(None if masks is None else _f32(masks)), n, h, w, c, ptr(sel_d[0]),
        None if flip is None else ptr(sel_d[1]), B, ptr(_f32(x)),
        ptr(None if gt is None else _f32(gt)), ptr(None if mask is None else _f32(mask)), stream())
    return x, gt, mask
