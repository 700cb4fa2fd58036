"""CPU tests of the C ABI boundary: the library loads and exports every declared symbol."""
import ctypes as C
import os
import subprocess

import pytest

from pldepth_amd import _lib


def test_library_exports_every_declared_symbol():
    lib = _lib.lib()
    declared = _lib.declared_symbols()
    assert len(declared) >= 30
    missing = [s for s in declared if not hasattr(lib._dll, s)]
    assert not missing, missing
    # every declared symbol has a ctypes signature, and vice versa
    assert set(declared) == set(_lib._SIGS), set(declared) ^ set(_lib._SIGS)


def test_exports_are_plain_c_symbols():
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    for s in _lib.declared_symbols():
        assert s in exported, s  # unmangled extern "C"


def test_library_exports_only_declared_symbols():
    """The header's "exports exactly the functions below": the cross-file pld__* helpers are
    hidden, so every exported pld_* text symbol is a declared entry point."""
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    exported = {s for s in exported if s.startswith("pld_")}
    assert not [s for s in exported if s.startswith("pld__")]
    assert exported == set(_lib.declared_symbols()), exported ^ set(_lib.declared_symbols())


P, I32, I64, U64 = C.c_void_p, C.c_int, C.c_int64, C.c_uint64
F32, F64, SZ = C.c_float, C.c_double, C.c_size_t


def test_binding_parsed_from_header_matches_pinned_layouts():
    """The structs, signatures and constants _lib reads from the header, against literals: both
    struct layouts, prototypes that together cover every mapped type, and one enumerator of each
    enum plus every #define."""
    assert _lib.ConvArgs._fields_ == [
        ("x1", P), ("x2", P), ("c1", I32), ("c2", I32),
        ("n", I32), ("h", I32), ("w", I32),
        ("kh", I32), ("kw", I32), ("sh", I32), ("sw", I32), ("pad_t", I32), ("pad_l", I32),
        ("oh", I32), ("ow", I32), ("cout", I32),
        ("in_scale", P), ("in_shift", P), ("in_act", I32), ("tile", I32),
        ("ws", P), ("ws_bytes", SZ), ("math", I32), ("w_split", P),
    ]
    assert _lib.RefreshDesc._fields_ == [
        ("w", P), ("w_nat", P), ("w_nat_split", P), ("w_dgrad", P), ("w_dgrad_split", P),
        ("taps", I32), ("cin", I32), ("cout", I32), ("blk0", I32), ("nblk", I32),
        ("reserved", I32),
    ]
    pinned = {
        "pld_dwconv_dgrad_se_bn": (I32, [P, P, I32, I32, I32, I32, P, I32, I32, I32, I32, I32, P,
                                         P, P, P, P, I32, P, P, P, I32, P, P, P, P, P, I32, P, P,
                                         I32, P, P, P, SZ, P]),
        "pld_adam_amsgrad": (I32, [P, P, P, P, P, I64, F32, F32, F32, F32, I64, F32, P]),
        "pld_graph_end": (I32, [P, C.POINTER(P)]),
        "pld_conv_schedule_desc": (C.c_char_p, [I32, I32]),
        "pld_dropconnect_scales_multi": (I32, [P, I32, I32, P, P, U64, U64, P, I32, P]),
        "pld_auto_canny_u8": (I32, [P, I32, I32, I32, F64, F64, P, P, P, P, P]),
        "pld_conv2d_wgrad": (I32, [C.POINTER(_lib.ConvArgs), P, P, I32, P, SZ, P]),
        "pld_conv2d_wgrad_workspace_size": (SZ, [C.POINTER(_lib.ConvArgs)]),
    }
    for name, sig in pinned.items():
        assert _lib._SIGS[name] == sig, name
    # status wrapping: by return type, and the int-valued queries by name
    assert {"pld_conv_schedule_desc", "pld_conv2d_wgrad_workspace_size", "pld_version",
            "pld_filter_refresh_plan"} <= _lib._NON_STATUS
    assert not _lib._NON_STATUS & {"pld_graph_end", "pld_adam_amsgrad", "pld_conv2d_wgrad"}
    assert len(_lib._NON_STATUS) == 28
    for name, value in {
            "PLD_ERR_UNSUPPORTED": 3, "PLD_ACT_SWISH": 2, "PLD_SAMPLER_INFO": 3,
            "PLD_MATH_BF16X3": 1, "PLD_SCHED_X3_HALO": 6, "PLD_KIND_DIRECT": 2,
            "PLD_EDGE_MAX_DIM": 512, "PLD_MEDIAN_MAX_KSIZE": 15, "PLD_TILE_MAX": 32,
            "PLD_ORACLE_MAX_L": 16, "PLD_DROPCONNECT_MAX_LAYERS": 32}.items():
        assert _lib.CONST[name] == value, name


@pytest.mark.parametrize("text", [
    "int pld_f(const foo_t* x, int n);",            # unknown type
    "foo_t pld_f(void);",
    "typedef struct pld_s { foo_t a; } pld_s;",
    "int pld_f(int a, int b\nint pld_g(void);",     # unterminated prototype
    "int pld_g(void);\nint pld_f(int a)",
    "enum { PLD_A, PLD_B };",                       # constructs the header does not use
    "#if 1\nint pld_f(void);\n#endif",
    "int pld_f(int (*cb)(int));",
])
def test_header_parser_raises_on_what_it_does_not_understand(text):
    assert _lib.parse_header("int pld_ok(const float* x, size_t n);")[1] == {
        "pld_ok": (I32, [P, SZ])}
    with pytest.raises(_lib.PLDError):
        _lib.parse_header(text)


def test_host_only_entry_points():
    lib = _lib.lib()
    assert lib.pld_version() == 1
    assert lib.pld_sampler_candidates(100, 3) == 500
    assert lib.pld_sampler_candidates(100, 0) == 80
    assert lib.pld_sampler_candidates(100, 2) == 150
    # argument validation fails loudly before touching the GPU
    try:
        lib.pld_listmle_fwd_bwd(None, None, 1, 1, 1, 1, None, None, None, 1, None)
    except _lib.PLDError as e:
        assert "null pointer" in str(e)
    else:
        raise AssertionError("expected PLDError")
    a = _lib.ConvArgs()
    assert lib.pld_conv2d_wgrad_workspace_size(C.byref(a)) == 0  # invalid geometry
    assert lib.pld_conv2d_fwd_workspace_size(C.byref(a)) == 0
    assert lib.pld_conv2d_dgrad_workspace_size(C.byref(a)) == 0
    # split-K schedules of a deep, small-M GEMM need a slab workspace; plain ones do not
    a.n, a.h, a.w, a.c1, a.kh, a.kw, a.sh, a.sw = 1, 7, 7, 1024, 3, 3, 1, 1
    a.pad_t = a.pad_l = 1
    a.oh, a.ow, a.cout = 7, 7, 64
    nt = lib.pld_conv_num_tiles()
    a.tile = 0
    assert lib.pld_conv2d_fwd_workspace_size(C.byref(a)) == 0
    a.tile = nt // 2
    assert lib.pld_conv2d_fwd_workspace_size(C.byref(a)) >= 2 * 49 * 64 * 4


def test_filter_refresh_plan_and_descriptor_layout():
    """pld_filter_refresh_plan (host arithmetic only): the block count of a filter's batched
    refresh, 0 where the batched path does not apply; the ctypes descriptor matches the
    header's pld_filter_refresh_desc (5 pointers + 6 ints = 64 B)."""
    from pldepth_amd import kernels as K
    lib = _lib.lib()
    p, q = C.c_void_p(1 << 20), C.c_void_p((1 << 20) + 4)  # 16-byte aligned / not
    # 3x3, 64 -> 64: 9 x 1 native tiles + ceil(576 * 64 / 8 / 256) = 18 dgrad blocks
    assert lib.pld_filter_refresh_plan(3, 3, 64, 64, p, p, p, p, p) == 9 + 18
    assert lib.pld_filter_refresh_plan(3, 3, 64, 64, p, p, None, None, None) == 9
    assert lib.pld_filter_refresh_plan(3, 3, 3, 32, p, p, p, p, p) == 0   # R = 27 % 8
    assert lib.pld_filter_refresh_plan(3, 3, 64, 100, p, p, p, p, p) == 0  # dgrad cout % 8
    assert lib.pld_filter_refresh_plan(3, 3, 64, 64, p, q, p, p, p) == 0   # misaligned
    assert lib.pld_filter_refresh_plan(3, 3, 64, 64, p, p, p, None, p) == 0  # split w/o dgrad
    assert C.sizeof(K._RefreshDesc) == 64
    with pytest.raises(_lib.PLDError):
        lib.pld_filter_refresh_multi(None, 1, 1, None)


def test_header_documents_reference_replacements():
    txt = open(_lib.HEADER).read()
    for ref in ["depth_utils.py:39-61", "nll_loss.py", "PLDepth.py:133", "pl_hourglass.py",
                "sampling.py"]:
        assert ref in txt, ref


def test_schedule_names_are_unique_and_resolve():
    """pld_conv_schedule_desc names every schedule once per math; the persisted table
    (kernels.DEFAULT_SCHEDULES) names only schedules this build has, for gfx950."""
    import json

    from pldepth_amd import kernels as K
    lib = _lib.lib()
    for math in K.MATH.values():
        n = lib.pld_conv_num_schedules(math)
        names = [lib.pld_conv_schedule_desc(math, i).decode() for i in range(n)]
        assert len(set(names)) == n, names
        assert lib.pld_conv_schedule_desc(math, n) is None
        assert all(K._schedule_index(math, d) == i for i, d in enumerate(names))
    if os.path.exists(K.DEFAULT_SCHEDULES):
        d = json.load(open(K.DEFAULT_SCHEDULES))
        assert d["format"] == K.SCHEDULE_FORMAT and d["arch"].startswith("gfx950")
        assert d["entries"]
        for key, desc in d["entries"]:
            assert len(key) == len(d["key"])
            assert K._schedule_index(key[-1], desc) is not None, (key, desc)
        # the same entries are taken on a gfx950 device (arch given: no GPU here)
        saved = dict(K._TILE_CACHE)
        try:
            K._TILE_CACHE.clear()
            assert K.load_tile_cache(K.DEFAULT_SCHEDULES, arch=d["arch"]) == len(d["entries"])
        finally:
            K._TILE_CACHE.clear()
            K._TILE_CACHE.update(saved)


def test_bench_self_spawn_command(monkeypatch):
    """bench.py --gpus N without a launcher runs torch.distributed.run with N ranks on
    127.0.0.1 as one child process and exits with its code (no GPU call in the parent)."""
    import subprocess as sp
    import sys

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    seen = {}

    def fake_call(cmd, env=None):
        seen["cmd"], seen["env"] = cmd, env
        return 7

    monkeypatch.setattr(sp, "call", fake_call)
    assert bench.spawn_ranks(8, ["--gpus", "8", "--steps", "3"]) == 7
    cmd = seen["cmd"]
    assert cmd[1:3] == ["-m", "torch.distributed.run"]
    assert cmd[cmd.index("--nproc-per-node") + 1] == "8"
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    assert cmd[-4:] == ["--gpus", "8", "--steps", "3"] and cmd[-5].endswith("bench.py")
