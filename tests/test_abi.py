"""CPU (`-m "not gpu"`): the C-ABI library loads, exports every symbol include/sympa_hip.h declares,
and validates arguments (no compute calls without a GPU)."""
import ctypes
import os
import re

import pytest

from sympa_amd import _lib
from tests.helpers import ROOT


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "sympa_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(sympa_[a-z_0-9]+)\s*\(", text)))


def test_header_matches_binding():
    assert declared_symbols() == sorted(_lib.SYMBOLS)


def test_library_exports_every_declared_symbol():
    lib = _lib.load()
    for s in declared_symbols():
        assert hasattr(lib, s), s
    assert b"gfx950" in lib.sympa_version()
    assert lib.sympa_max_dims() == 8


def test_argument_validation_without_gpu():
    lib = _lib.load()
    one = ctypes.c_void_p(16)   # never dereferenced: validation happens before any launch
    # b == 0 is a no-op
    assert lib.sympa_siegel_dist_fwd(one, one, 0, 4, 0, 0, None, 1e-5, one, None, None, 0, None) == 0
    assert lib.sympa_siegel_dist_fwd(one, one, -1, 4, 0, 0, None, 1e-5, one, None, None, 0, None) == -1
    assert lib.sympa_siegel_dist_fwd(None, one, 8, 4, 0, 0, None, 1e-5, one, None, None, 0, None) == -1
    assert lib.sympa_siegel_dist_fwd(one, one, 8, 4, 7, 0, None, 1e-5, one, None, None, 0, None) == -1   # model
    assert lib.sympa_siegel_dist_fwd(one, one, 8, 4, 0, 9, None, 1e-5, one, None, None, 0, None) == -1   # metric
    assert lib.sympa_siegel_dist_fwd(one, one, 8, 4, 0, 4, None, 1e-5, one, None, None, 0, None) == -1   # wsum w/o w
    assert lib.sympa_siegel_dist_fwd(one, one, 8, 4, 0, 0, None, 0.0, one, None, None, 0, None) == -1    # eps
    assert lib.sympa_siegel_dist_fwd(one, one, 8, 99, 0, 0, None, 1e-5, one, None, None, 0, None) == -2  # dims
    assert b"dims" in lib.sympa_last_error()
    assert lib.sympa_model_forward(one, 10, 4, None, 2, one, 2, 8, 0, 0, None, 1e-5, None, 1.0, one, None, 0, None) == -1
    assert lib.sympa_model_forward(one, 0, 4, one, 2, one, 2, 8, 0, 0, None, 1e-5, None, 1.0, one, None, 0, None) == -1


def test_digest_and_refresh_entries_validate_their_arguments_without_gpu():
    lib = _lib.load()
    one, al = ctypes.c_void_p(8), ctypes.c_void_p(64)   # never dereferenced
    assert lib.sympa_table_digest(None, 64, al, 0, None) == -1
    assert lib.sympa_table_digest(al, 64, None, 0, None) == -1
    assert lib.sympa_table_digest(al, 0, al, 0, None) == -1
    assert lib.sympa_table_digest(al, 12, al, 0, None) == -1          # not a multiple of 8
    assert lib.sympa_table_digest(one, 64, al, 0, None) == -1         # data not 16-byte aligned
    assert lib.sympa_table_pack_refresh(al, 10, 4, 0, al, 1 << 20, al, 0, None, None) == -2      # dims outside 5..8
    assert lib.sympa_table_pack_refresh(al, 10, 8, 0, al, 1 << 20, None, 0, None, None) == -1    # no digest state
    assert lib.sympa_table_pack_refresh(al, 0, 8, 0, al, 1 << 20, al, 0, None, None) == -1       # empty table
    assert lib.sympa_spd_table_pack_refresh(al, 10, 3, al, 1 << 20, al, 0, None, None) == -2
    assert lib.sympa_spd_table_pack_refresh(al, 10, 16, al, 1 << 20, None, 0, None, None) == -1


def test_merged_rows_flag_is_refused_where_no_kernel_honours_it():
    """SYMPA_FLAG_MERGE_SRC with per-pair rows (round-5 advice): only the one-lane kernels of dims <= 6 write the merged layout; the
    split / eight-lanes / dims >= 7 kernels would write every row while the caller's slot list drops all but the run ends."""
    lib = _lib.load()
    one = ctypes.c_void_p(16)   # never dereferenced: refused before any launch
    D = ctypes.c_double
    MERGE, SPLIT, COOP = 128, 64, 32

    def call(n, flags, rows=True):
        return lib.sympa_model_train_backward(one, 100, n, one, 2, one, 2, one, 64, None, 0, 0, None, D(1e-5), None, D(1.0), D(1.0),
                                              one, None if rows else one, one if rows else None, None, None, None, None, None, 0,
                                              flags, None)
    assert call(8, MERGE) == -1 and b"MERGE_SRC" in lib.sympa_last_error()
    assert call(7, MERGE) == -1
    assert call(6, MERGE | SPLIT) == -1 and call(5, MERGE | COOP) == -1


def test_radam_entry_points_validate_their_arguments_without_gpu():
    lib = _lib.load()
    one = ctypes.c_void_p(16)   # never dereferenced: validation happens before any launch
    D = ctypes.c_double
    # rows == 0 is a no-op; null state, bad betas, dims outside 1..6 are refused
    assert lib.sympa_radam_step(one, one, one, one, 0, 4, 0, D(0.1), D(0.9), D(0.999), D(1e-7), D(0.0), one, D(1e-5), None, None, None) == 0
    assert lib.sympa_radam_step(one, one, None, one, 8, 4, 0, D(0.1), D(0.9), D(0.999), D(1e-7), D(0.0), one, D(1e-5), None, None, None) == -1
    assert lib.sympa_radam_step(one, one, one, one, 8, 4, 0, D(0.1), D(1.0), D(0.999), D(1e-7), D(0.0), one, D(1e-5), None, None, None) == -1
    assert lib.sympa_radam_step(one, one, one, one, 8, 4, 7, D(0.1), D(0.9), D(0.999), D(1e-7), D(0.0), one, D(1e-5), None, None, None) == -1
    assert lib.sympa_radam_step(one, one, one, one, 8, 7, 0, D(0.1), D(0.9), D(0.999), D(1e-7), D(0.0), one, D(1e-5), None, None, None) == -2
    assert b"dims" in lib.sympa_last_error()
    # the fused step: null Adam state / empty table before anything touches a device
    assert lib.sympa_radam_step_fused(one, one, None, one, one, 8, 4, 0, D(0.1), D(0.9), D(0.999), D(1e-7), D(0.0), D(1e-5), D(1.0), 1,
                                      None, None, None, None, None, None, None, None, 0, one, 64, None, 0, None, None, None, None) == -1
    assert lib.sympa_radam_step_fused(one, one, one, one, one, 0, 4, 0, D(0.1), D(0.9), D(0.999), D(1e-7), D(0.0), D(1e-5), D(1.0), 1,
                                      None, None, None, None, None, None, None, None, 0, one, 64, None, 0, None, None, None, None) == -1


def test_product_path_refuses_cpu_tensors():
    import torch
    from sympa_amd import ops
    z = torch.zeros(2, 2, 3, 3, dtype=torch.float64)
    with pytest.raises(_lib.SympaHipError):
        ops.siegel_dist_forward(z, z)
    with pytest.raises(_lib.SympaHipError):
        ops.model_forward(z, torch.zeros(2, 2, dtype=torch.int64))


def test_missing_library_fails_loudly(monkeypatch):
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", "/nonexistent/libsympa_hip.so")
    with pytest.raises(_lib.SympaHipError):
        _lib.load()


def test_integration_md_stub_compiles_and_matches_the_binding():
    """INTEGRATION.md section 3 shows the ctypes stub a maintainer of the reference would paste into
    sympa/manifolds/siegel_manifold.py.  Extract it, execute it (stand-ins for the two names the reference file
    already has in scope) and check its prototypes against this package's own binding, and that it only uses
    attributes the reference's class really has (self.dims, self.metric -- there is no metric_name)."""
    import re
    from abc import ABC
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    sec = text[text.index("## 3."):text.index("### 3b.")]      # 3b shows the loops around the path, not the ctypes stub
    blocks = re.findall(r"```python\n(.*?)```", sec, flags=re.S)
    assert len(blocks) == 1
    src = blocks[0]
    assert "metric_name" not in src and "self.metric" in src and "self.dims" in src
    cwd = os.getcwd()
    os.chdir(ROOT)                  # the stub loads the library by its in-tree relative path
    try:
        ns = {"Manifold": type("Manifold", (), {}), "ABC": ABC}   # geoopt's base class stands in
        exec(compile(src, "INTEGRATION.md#3", "exec"), ns)
    finally:
        os.chdir(cwd)
    lib = _lib.load()
    for name in ("sympa_siegel_dist_fwd", "sympa_siegel_dist_bwd"):
        assert list(getattr(ns["_lib"], name).argtypes) == list(getattr(lib, name).argtypes), name
        assert getattr(ns["_lib"], name).restype is getattr(lib, name).restype
    # the class-name -> id table covers exactly the mirror's metric classes, with the C-ABI's ids
    from sympa_amd.manifolds import metrics as mm
    from sympa_amd.ops import METRIC_IDS
    for t in mm.MetricType:
        cls = type(mm.Metric.get(t, 3)).__name__
        assert ns["_METRIC_ID"][cls] == METRIC_IDS[t.value], cls
    assert hasattr(ns["SiegelManifold"], "dist") and ns["SiegelManifold"].model_id == 0


def test_every_translation_unit_passed_the_dpp_hazard_scan():
    """__graft_entry__.build() scans the gfx950 assembly of every unit it compiles (__graft_entry__.hip_units(): the plain .hip
    files and one unit per line of csrc/siegel_bwd_instances.hpp) for the DPP hazards the compiler cannot see in inline asm
    (tools/check_dpp_hazards.py) and rebuilds a unit that fails with the wait states inside the asm statements; its report must
    list every unit as clean in the end.  No .hip file of csrc/ may stay outside the units."""
    import os
    import __graft_entry__ as entry
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sympa_amd", "csrc")
    units = entry.hip_units()
    assert {src for _, src, _ in units} == {f for f in os.listdir(csrc) if f.endswith(".hip")}
    report = os.path.join(csrc, "dpp_hazard_report.txt")
    if not os.path.exists(os.path.join(csrc, "libsympa_hip.so")):
        import pytest
        pytest.skip("library not built in this tree")
    # a built tree WITHOUT the report was not built by the one supported path (__graft_entry__.build_hip, which
    # `make -C sympa_amd/csrc` forwards to): it may contain the hazardous units -- a failure, not a skip
    assert os.path.exists(report), "libsympa_hip.so exists but dpp_hazard_report.txt does not: built outside __graft_entry__.build()"
    lines = {l.split()[0]: l.strip() for l in open(report) if l.strip() and not l.startswith("#")}
    assert sorted(lines) == [name for name, _, _ in units]
    dpp = {u: l.split(";")[0].strip() for u, l in lines.items()}
    assert all(l.endswith("clean") for l in dpp.values()), [l for l in dpp.values() if not l.endswith("clean")]
    # ... and (round 5, tools/dma_reload_check.py) no LDS-DMA instruction of any unit sits behind a scratch reload: such a reload
    # is followed by s_waitcnt vmcnt(0) and serialises the gather, one round trip per row
    import re
    for u, l in lines.items():
        m = re.search(r"(\d+) LDS-DMA instructions, (\d+) behind a scratch reload", l)
        assert m, f"{u}: no LDS-DMA scan in the report (rebuild with __graft_entry__.build())"
        assert int(m.group(2)) == 0, l


def test_the_instance_list_is_the_cross_product_of_every_family():
    """csrc/siegel_bwd_instances.hpp, read the way the build reads it, against the families restated here: every backward kernel
    with a compile job of its own, once, and no unit name taken twice.  (The list also makes the declarations and the dispatch:
    a wrapper the dispatch names and no unit defines fails when build() loads the library, which binds every symbol.)"""
    import __graft_entry__ as entry
    forms = ("dense", "scatter")
    want = [("COOP", m, n, f) for m in ("upper", "bounded") for n in range(9, 17) for f in forms]
    want += [("HALF", m, n, f) for m in ("upper", "bounded") for n in range(5, 9) for f in forms]
    want += [("SPLIT_SPECTRAL", m, n, None) for m in ("upper", "bounded") for n in range(5, 9)]
    want += [("SPLIT_GRADIENT", m, n, f) for m in ("upper", "bounded") for n in range(5, 9) for f in forms]
    want += [("ONE_LANE", m, n, f) for m in ("upper", "bounded", "dual") for n in (7, 8) for f in forms]
    got = entry.bwd_instances()
    assert len(got) == len(set(got)) == 84
    assert set(got) == set(want)
    units = entry.hip_units()
    names = [name[:-4] if name.endswith(".hip") else name for name, _, _ in units]
    assert len(set(names)) == len(names)                    # one object file per unit
    instances = [u for u in units if u[2]]
    assert len(instances) == 84 and len({tuple(d) + (src,) for _, src, d in instances}) == 84
    assert {"siegel_bwd_coop_upper_9_dense", "siegel_bwd_half_bounded_8_scatter", "siegel_bwd_split_spectral_upper_5",
            "siegel_bwd_split_gradient_bounded_6_dense", "siegel_bwd_n7_dual_scatter"} <= {name for name, _, _ in instances}


# ---- the ctypes prototypes and the constants are read from the header (sympa_amd/_lib.py::parse_header) --------------------

_TYPE_NAME = {getattr(ctypes, n): n for n in ("c_int", "c_int64", "c_double", "c_void_p", "c_char_p")}


def _type_names(fn):
    return [_TYPE_NAME[fn.restype], [_TYPE_NAME[t] for t in fn.argtypes or ()]]


def test_prototypes_equal_the_recorded_hand_written_table():
    """tests/golden/abi_prototypes.json was recorded from the hand-written argtypes table this binding used to carry (never from
    the parser): every entry it names is still declared and keeps exactly those types on the loaded handle.  An ABI-stability
    lock for the 71 entries of that day, not a mirror: later entries need not be added."""
    import json
    recorded = json.load(open(os.path.join(ROOT, "tests", "golden", "abi_prototypes.json")))
    assert len(recorded) == 71
    lib = _lib.load()
    for name, types in recorded.items():
        assert name in _lib.SYMBOLS, name
        assert _type_names(getattr(lib, name)) == types, name


def test_arity_counted_by_an_independent_reader():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sympa_hip.h")).read(), flags=re.S)
    args = dict(re.findall(r"\b(sympa_[a-z_0-9]+)\s*\(([^)]*)\)", text))
    assert sorted(args) == declared_symbols() and len(args) >= 71
    lib = _lib.load()
    for name, a in args.items():
        fn = getattr(lib, name)
        assert len(fn.argtypes or ()) == (0 if a.strip() == "void" else a.count(",") + 1), name
        assert fn.restype in (ctypes.c_int, ctypes.c_int64, ctypes.c_char_p), name   # set for every entry (the default is c_int)
        assert _lib.PROTOTYPES[name][0] is fn.restype, name


def test_one_prototype_of_every_type_shape():
    lib = _lib.load()
    P, L, I, D = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_double
    assert not lib.sympa_version.argtypes and lib.sympa_version.restype is ctypes.c_char_p
    assert list(lib.sympa_table_pack_bytes.argtypes) == [L, I, I] and lib.sympa_table_pack_bytes.restype is L
    batches = lib.sympa_model_forward_batches.argtypes
    assert batches[3] is P and batches[13] is P and batches[16] is P    # const int64_t* const*, double* const*, void* const*
    assert list(batches) == [P, L, I, P, L, P, I, I, I, P, D, P, D, P, P, I, P, I]
    fused = list(lib.sympa_radam_step_fused.argtypes)
    assert len(fused) == 33 and fused[8:15] == [D] * 7
    assert fused == [P, P, P, P, P, L, I, I, D, D, D, D, D, D, D, I, P, P, P, P, P, P, P, P, I, P, L, P, I, P, P, P, P]
    assert lib.sympa_radam_step_fused.restype is I


@pytest.mark.parametrize("text", [
    "int sympa_x(float a);",                        # a by-value type outside the table
    "int sympa_x(struct s a);",
    "double* sympa_x(void);",                       # a pointer return other than const char*
    "int sympa_x(int a, double b",                  # cut off before );
    "int sympa_y(int a);\nint sympa_x(int64_t b, const double* c",
])
def test_the_parser_refuses_what_it_cannot_type(text):
    with pytest.raises(_lib.SympaHipError, match="sympa_x"):
        _lib.parse_header(text)


def test_the_parser_reads_declarations_and_defines_and_skips_comments():
    protos, defines = _lib.parse_header(
        "/* int sympa_old(float a); sympa_model_forward(...) */\n#ifndef SYMPA_HIP_H\n#define SYMPA_HIP_H\n"
        "#define SYMPA_A 7 /* seven,\n  sympa_b(  */\n#define SYMPA_ERR (-2)\n"
        "const char* sympa_v(void);\nint64_t sympa_w(const int64_t* const* a, int b,\n   double c, int64_t d, void* const* e);\n#endif\n")
    assert list(protos.items()) == [("sympa_v", (ctypes.c_char_p, [])), ("sympa_w", (ctypes.c_int64, [
        ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_int64, ctypes.c_void_p]))]
    assert defines == {"SYMPA_A": 7, "SYMPA_ERR": -2}


def test_a_missing_header_fails_loudly(monkeypatch):
    monkeypatch.setattr(_lib, "HEADER_PATH", "/nonexistent/sympa_hip.h")
    with pytest.raises(_lib.SympaHipError, match="sympa_hip.h not found"):
        _lib.read_header()


def test_constants_keep_their_values():
    from sympa_amd import ops, selfcheck
    assert (ops.FLAG_LOW_LDS, ops.FLAG_GENERIC, ops.FLAG_ANY_ORDER, ops.FLAG_FUSE, ops.FLAG_NO_SYMMETRY, ops.FLAG_COOP, ops.FLAG_SPLIT,
            ops.FLAG_MERGE_SRC, ops.FLAG_FP32_KEYS) == (1, 2, 4, 8, 16, 32, 64, 128, 256)
    assert (ops.ST_NOT_PD, ops.ST_NONFINITE, ops.ST_BAD_INDEX, ops.ST_NO_CONVERGENCE) == (1, 2, 4, 8)
    assert ops.MAX_FUSED_BATCHES == 32 and ops.MAP_LDS_CAP == 1024
    assert ops.MODEL_IDS == {"upper": 0, "bounded": 1, "dual": 2}
    assert ops.METRIC_IDS == {"riem": 0, "fone": 1, "finf": 2, "fmin": 3, "wsum": 4}
    assert ops.VECTOR_MODEL_IDS == {"euclidean": 0, "poincare": 1, "lorentz": 2, "sphere": 3, "prod-hysph": 4, "prod-hyhy": 5,
                                    "prod-hyeu": 6, "prod-sphsph": 7}
    assert (selfcheck.SIEGEL_FWD, selfcheck.SIEGEL_BWD, selfcheck.SIEGEL_TABLE, selfcheck.SPD_FWD, selfcheck.SPD_BWD,
            selfcheck.SPD_TABLE) == (0, 1, 2, 3, 4, 5)
    assert selfcheck.MODEL_IDS == {"upper": 0, "bounded": 1, "spd": 0}
    assert all(type(v) is int for v in _lib.DEFINES.values()) and "SYMPA_HIP_H" not in _lib.DEFINES


def test_bind_types_a_second_handle_and_names_a_missing_symbol():
    lib = _lib.load()
    other = ctypes.CDLL(_lib.LIB_PATH)
    assert other is not lib and other.sympa_model_forward.argtypes is None
    assert _lib.bind(other) is other
    for name in _lib.SYMBOLS:
        assert _type_names(getattr(other, name)) == _type_names(getattr(lib, name)), name

    class Partial:
        pass
    for name in _lib.SYMBOLS:
        if name != "sympa_map_rows":
            setattr(Partial, name, staticmethod(lambda: None))
    with pytest.raises(_lib.SympaHipError, match="does not export sympa_map_rows"):
        _lib.bind(Partial())
