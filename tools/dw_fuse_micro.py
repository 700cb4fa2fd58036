"""Time the MBConv backward from the SE output's gradient to the expand BN's coefficients at the
stride-1 block shapes of ff_effnet 448x448 batch 32, in its four wirings:

    pair  pld_se_bwd_bn_full -> pld_dwconv_dgrad -> pld_bn_bwd_coeffs            (unfused)
    pro   pld_se_bwd_bn_coeffs -> pld_dwconv_dgrad_se_bn (no ex) -> pld_bn_bwd_coeffs
    epi   pld_se_bwd_bn_full -> pld_dwconv_dgrad_bn_bwd
    both  pld_se_bwd_bn_coeffs -> pld_dwconv_dgrad_se_bn (ex)

Each wiring is captured into a hipGraph of ITERS repeats and replayed REPS times; the table gives
the median microseconds per repeat and the spread (max - min) over the replays. Block 1a has no
expand conv: its rows stop at the dgrad, and epi / both do not apply.

    python tools/dw_fuse_micro.py [--iters 10] [--reps 7]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# (blocks, map side, expanded channels, kernel, squeeze channels, has an expand conv)
SHAPES = [("1a", 224, 32, 3, 8, False), ("2b", 112, 144, 3, 6, True),
          ("3b", 56, 240, 5, 10, True), ("4b 4c", 28, 480, 3, 20, True),
          ("5a", 28, 480, 5, 20, True), ("5b 5c", 28, 672, 5, 28, True),
          ("6b 6c 6d", 14, 1152, 5, 48, True), ("7a", 14, 1152, 3, 48, True)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--n", type=int, default=32)
    a = ap.parse_args()
    from pldepth_amd import kernels as K
    torch.cuda.set_device(0)
    g = torch.Generator(device="cuda").manual_seed(0)
    n = a.n
    print(f"{'blocks':9s} {'shape':18s}" + "".join(f"{v:>18s}" for v in ("pair", "pro", "epi", "both"))
          + "   (median us +- spread)")
    with torch.cuda.stream(torch.cuda.Stream()):
        for name, hw, c, k, cse, has_ex in SHAPES:
            r = lambda *s: torch.randn(*s, device="cuda", generator=g)
            vec = lambda: (r(c) * 0.1, torch.rand(c, device="cuda", generator=g) + 0.5, r(c), r(c))
            gse, dw_pre, ex = r(n, hw, hw, c), r(n, hw, hw, c), r(n, hw, hw, c)
            gdw, ge = torch.empty_like(gse), torch.empty_like(gse)
            bn, ebn = vec(), vec()
            w1, w2, wdw = r(c, cse) * 0.1, r(cse, c) * 0.1, r(k, k, c) / k
            z1, gate = r(n, cse), torch.rand(n, c, device="cuda", generator=g)
            e = lambda *s: torch.empty(*s, device="cuda")
            addn, dg, db, bk12, edg, edb, ek12 = e(n, c), e(c), e(c), e(2 * c), e(c), e(c), e(2 * c)
            p = k // 2
            rows = n * hw * hw

            def full():
                K.se_bwd_bn_full(gse, dw_pre, bn, w1, w2, z1, gate, addn, gdw, dg, db)

            def coeffs():
                K.se_bwd_bn_coeffs(gse, dw_pre, bn, w1, w2, z1, gate, addn, dg, db, bk12)

            def ebn_coeffs():
                if has_ex:
                    K.bn_bwd_coeffs(ex, ge, rows, c, *ebn, "swish", edg, edb, ek12)

            def pair():
                full()
                K.dwconv_dgrad(gdw, wdw, k, 1, p, p, ge)
                ebn_coeffs()

            def pro():
                coeffs()
                K.dwconv_dgrad_se_bn(gse, dw_pre, bn, bk12, gate, addn, wdw, k, p, p, ge)
                ebn_coeffs()

            def epi():
                full()
                K.dwconv_dgrad_bn_bwd(gdw, wdw, k, 1, p, p, ge, ex, ebn, "swish", edg, edb, ek12)

            def both():
                coeffs()
                K.dwconv_dgrad_se_bn(gse, dw_pre, bn, bk12, gate, addn, wdw, k, p, p, ge, ex=ex,
                                     ebn=ebn, edgamma=edg, edbeta=edb, ek12=ek12)

            cells = []
            for fn in (pair, pro, epi, both):
                if not has_ex and fn in (epi, both):
                    cells.append(f"{'-':>18s}")
                    continue
                fn()  # workspaces allocated before the capture
                torch.cuda.synchronize()
                gr = K.Graph().capture(lambda: [fn() for _ in range(a.iters)])
                gr.launch()
                torch.cuda.synchronize()
                ts = []
                for _ in range(a.reps):
                    e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
                    e0.record()
                    gr.launch()
                    e1.record()
                    e1.synchronize()
                    ts.append(e0.elapsed_time(e1) / a.iters * 1e3)
                ts.sort()
                cells.append(f"{ts[len(ts) // 2]:10.1f} +- {ts[-1] - ts[0]:4.1f}")
                del gr
            print(f"{name:9s} {n}x{hw}x{hw}x{c} k{k}".ljust(28) + "".join(cells), flush=True)
            del gse, dw_pre, ex, gdw, ge
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
