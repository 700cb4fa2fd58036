"""Time the fused pgemm calls against the unfused pairs they replace at the ff_effnet 448x448
batch-32 shapes (project convs over BN+swish+gate, expand dgrads over the BN backward):
pld_pgemm_bn_act / _bn_bwd (exact fp32, early blocks) and pld_pgemm_x3_bn_act / _bn_bwd (bf16x3
MFMA, blocks 3a-7a). Each variant is captured into a graph of INNER calls and replayed; the
figure is the median replay per call, the spread the largest difference between two replays.

    python tools/pgemm_micro.py [--family fp32|x3|all] [--iters 20]
"""
import argparse
import os
import statistics
import sys

import torch  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (name, images, hw, K = cexp, N): project convs (fwd) and expand dgrads (bwd)
SHAPES = [("1a_proj", 32, 224 * 224, 32, 16), ("2a_proj", 32, 112 * 112, 96, 24),
          ("2b_proj", 32, 112 * 112, 144, 24), ("3a_proj", 32, 56 * 56, 144, 40),
          ("3b_proj", 32, 56 * 56, 240, 40),
          ("2a_exdg", 32, 224 * 224, 96, 16), ("2b_exdg", 32, 112 * 112, 144, 24),
          ("3a_exdg", 32, 112 * 112, 144, 24), ("3b_exdg", 32, 56 * 56, 240, 40),
          ("4a_exdg", 32, 56 * 56, 240, 40)]
# the deep-K blocks (one line per distinct shape; the blocks that share it are named together).
# The expand dgrads are timed in their accumulating form (most of these blocks are residual)
X3_SHAPES = [("3a_proj", 32, 56 * 56, 144, 40), ("3b_proj", 32, 56 * 56, 240, 40),
             ("4a_proj", 32, 28 * 28, 240, 80), ("4bc_proj", 32, 28 * 28, 480, 80),
             ("5a_proj", 32, 28 * 28, 480, 112), ("5bc_proj", 32, 28 * 28, 672, 112),
             ("6a_proj", 32, 14 * 14, 672, 192), ("6bcd_proj", 32, 14 * 14, 1152, 192),
             ("7a_proj", 32, 14 * 14, 1152, 320),
             ("3b4a_exdg", 32, 56 * 56, 240, 40), ("4bc5a_exdg", 32, 28 * 28, 480, 80),
             ("5bc6a_exdg", 32, 28 * 28, 672, 112), ("6bcd7a_exdg", 32, 14 * 14, 1152, 192)]
INNER = 5


def timeit(fn, iters):
    """(median, spread) in ms per call of `fn`, graph-replayed."""
    from pldepth_amd import kernels as K
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        fn()  # warm-up outside the capture: autotunes the conv, sizes the workspaces
        st.synchronize()
        g = K.Graph().capture(lambda: [fn() for _ in range(INNER)])
        g.launch()
        st.synchronize()
        t = []
        for _ in range(iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            g.launch()
            e1.record(st)
            e1.synchronize()
            t.append(e0.elapsed_time(e1) / INNER)
    return statistics.median(t), max(t) - min(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--family", choices=("fp32", "x3", "all"), default="all")
    a = ap.parse_args()
    from pldepth_amd import kernels as K
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    todo = []
    if a.family in ("fp32", "all"):
        todo += [(s, False) for s in SHAPES]
    if a.family in ("x3", "all"):
        todo += [(s, True) for s in X3_SHAPES]
    for (name, n, hw, k, nn), x3 in todo:
        rows = n * hw
        x = torch.randn(n, hw, 1, k, device=dev, generator=g)
        bn = [torch.rand(k, device=dev, generator=g) + 0.5 for _ in range(4)]
        y = torch.empty(n, hw, 1, nn, device=dev)
        w = torch.randn(nn, 1, 1, k, device=dev, generator=g)
        K.filter_split(w)
        if name.endswith("proj"):
            gate = torch.rand(n, k, device=dev, generator=g)
            call = K.pgemm_x3_bn_act if x3 else K.pgemm_bn_act
            fused = lambda: call(x, rows, k, *bn, "swish", w, nn, y, gate=gate, hw=hw)
            a_ = torch.empty_like(x)
            args = K.conv_args(a_, None, 1, 1, 1, 0, 0, hw, 1, nn, math="bf16x3")

            def unfused():
                K.bn_apply(x, rows, k, *bn, "swish", a_, gate=gate, hw=hw)
                K.conv2d_fwd(args, w, None, y)
            by = 4.0 * rows * (k + nn)
        else:
            dy = torch.randn_like(x)
            k12 = torch.randn(2 * k, device=dev, generator=g) * 0.01
            dg, db = torch.empty(k, device=dev), torch.empty(k, device=dev)
            acc = x3
            call = K.pgemm_x3_bn_bwd if x3 else K.pgemm_bn_bwd

            def fused():  # the reductions stay: only the apply pass is folded
                K.bn_bwd_coeffs(x, dy, rows, k, *bn, "swish", dg, db, k12)
                call(x, dy, rows, k, *bn, "swish", k12, w, nn, y, accumulate=acc)
            gpe = torch.empty_like(x)
            args = K.conv_args(y, None, 1, 1, 1, 0, 0, hw, 1, k, math="bf16x3")

            def unfused():
                K.bn_bwd(x, dy, rows, k, *bn, "swish", gpe, dg, db)
                K.conv2d_dgrad(args, gpe, w, y, acc1=acc)
            by = 4.0 * rows * (2 * k + nn)
        tu, su = timeit(unfused, a.iters)
        tf, sf = timeit(fused, a.iters)
        print(f"{name:12s} rows {rows:8d} K {k:4d} N {nn:3d}: fused {tf * 1e3:7.1f} us "
              f"(+-{sf * 1e3:4.1f}, {by / tf / 1e9:5.2f} TB/s)   unfused {tu * 1e3:7.1f} us "
              f"(+-{su * 1e3:4.1f})   saved {(tu - tf) * 1e3:6.1f} us", flush=True)


if __name__ == "__main__":
    main()
