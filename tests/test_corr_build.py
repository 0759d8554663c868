"""Correlated noise, compile side (c3sc_hip_model_compile_cd / c3sc_hip_model_code_object_cd): no GPU is needed.
The new symbols are exported; a correlated model's code object is for gfx950 and holds the corr forms of the per-wave kernels
that the other flags select (at rank 12 the L2 form too) next to the forms without the term, never a rollout form, with no
private segment at ranks 4 and 8; ncorr = 0 yields the _ic code object instruction for instruction and needs no covar in the
source; a bad pair list is an argument error, pairs with a game, the box or interventions are refused; the library itself holds
no corr kernel and keeps its 666 entries; KArgs keeps its size."""
import ctypes as C
import os
import subprocess
import sys

import pytest

from c3sc_amd import engine as E
import corr_lib as CL
import impulse_lib as IL
import jump_lib as JL
import stop_lib as SL
from test_rtc_model_build import READELF, _bodies, _meta

ERR_ARG, ERR_UNSUPPORTED = 1, 3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (source, d, du, masks, pairs, njump)
MODELS = {"lqr": (CL.LQR, 2, 2, CL.LQR_MASKS, CL.LQR_PAIRS, 0), "lqr_jump": (CL.LQR_JUMP, 2, 2, CL.LQR_MASKS, CL.LQR_PAIRS, JL.LQR_NJUMP),
          "lqr3": (CL.LQR3, 3, 3, CL.LQR3_MASKS, CL.LQR3_PAIRS, 0)}


def _co(tmp_path_factory, model, tag, **kw):
    src, d, du, masks, pairs, nj = MODELS[model]
    co = E.code_object(src, d, du, name=f"{model}_{tag}", njump=nj, corr_pairs=pairs, **masks, **kw)
    p = tmp_path_factory.mktemp("co") / f"{model}_{tag}.co"
    p.write_bytes(co)
    return p


def test_new_symbols_are_exported_with_plain_c_names():
    L = E.load_library()
    for n in ("c3sc_hip_model_compile_cd", "c3sc_hip_model_code_object_cd", "c3sc_hip_set_correlation"):
        assert hasattr(L, n), n
        assert n in E.EXPORTS, n
    assert E.CORR_MAX == CL.CORR_MAX == 8
    assert E.STATUS_DOMINANCE == CL.STATUS_DOMINANCE == 4


def _corr(m, inner):
    """the corr kernels over the wrapped model `inner` (the mangled name that follows CorrOf<)"""
    return [k for k in m if "6CorrOfINS_" + inner in k]


def _expect_forms(names, ranks):
    for rp in ranks:
        for npl in (1, 2):
            for staged in ((1,) if rp < 12 else (0, 1)):
                n = sum("k_fiber_per_wave" in k and f"ELi{rp}ELi{npl}ELb0ELb0ELb{staged}E" in k for k in names)
                assert n == 1, (rp, npl, staged, n)
    assert not any("k_rollout" in k for k in names), "no rollout has a corr form"
    assert len(names) == sum(2 if rp < 12 else 4 for rp in ranks), names


def _gfx950(co):
    hdr = subprocess.run([READELF, "-h", str(co)], check=True, capture_output=True, text=True).stdout
    assert "EM_AMDGPU" in hdr and "gfx950" in hdr


def _no_private_segment(m):
    for name, priv in m.items():
        if "k_fiber_per_wave" in name:
            assert priv == 0, f"{name}: private segment of {priv} bytes"


def _vgprs(path):
    """{kernel name: VGPRs} of the per-wave kernels of a code object, from its metadata notes"""
    import re

    text = subprocess.run([READELF, "--notes", str(path)], check=True, capture_output=True, text=True).stdout
    out = {}
    for blk in text.split("- .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        if "k_fiber_per_wave" in name:
            out[name] = int(re.search(r"\.vgpr_count:\s+(\d+)", blk).group(1)), int(re.search(r"\.vgpr_spill_count:\s+(\d+)", blk).group(1))
    return out


def _within_two_workgroups_per_cu(co):
    """__launch_bounds__(256, 2) gives a lane 256 registers: every per-wave form stays inside them without a spill"""
    regs = _vgprs(co)
    assert regs
    for name, (v, spilled) in regs.items():
        assert v <= 256 and spilled == 0, (name, v, spilled)


def test_corr_code_object_plain(tmp_path_factory):
    co = _co(tmp_path_factory, "lqr", "cd", ranks=(4, 8))
    _gfx950(co)
    m = _meta(co)
    _expect_forms(_corr(m, "8RtcModel"), (4, 8))
    assert len([k for k in m if "CorrOf" in k]) == 2 * 2
    assert len([k for k in m if "RtcModel" in k and "CorrOf" not in k]) == 2 * 4  # the forms without the term, as the _ic spec gives them
    _no_private_segment(m)


def test_corr_code_object_with_horizon_and_stop(tmp_path_factory):
    co = _co(tmp_path_factory, "lqr", "cd_hs", ranks=(4, 8), horizon=True, stop=True)
    _gfx950(co)
    m = _meta(co)
    _expect_forms(_corr(m, "8RtcModel"), (4, 8))
    _expect_forms(_corr(m, "9HorizonOfINS_8RtcModel"), (4, 8))
    _expect_forms(_corr(m, "6StopOfINS_8RtcModel"), (4, 8))
    _expect_forms(_corr(m, "6StopOfINS_9HorizonOfINS_8RtcModel"), (4, 8))
    assert len([k for k in m if "CorrOf" in k]) == 4 * 2 * 2
    assert not any("k_rollout" in k and "CorrOf" in k for k in m)
    _no_private_segment(m)


def test_corr_code_object_with_njump(tmp_path_factory):
    co = _co(tmp_path_factory, "lqr_jump", "cd_j", ranks=(4, 8))
    _gfx950(co)
    m = _meta(co)
    _expect_forms(_corr(m, "8RtcModel"), (4, 8))
    _expect_forms(_corr(m, "6JumpOfINS_8RtcModel"), (4, 8))
    assert len([k for k in m if "CorrOf" in k]) == 2 * 2 * 2
    assert len([k for k in m if "JumpOf" in k and "CorrOf" not in k]) == 2 * 3  # the jump forms keep their rollouts
    _no_private_segment(m)


def test_corr_forms_at_rank_12_include_the_l2_per_wave_kernel(tmp_path_factory):
    co = _co(tmp_path_factory, "lqr", "cd_r12", ranks=(12,))
    m = _meta(co)
    _expect_forms(_corr(m, "8RtcModel"), (12,))
    _no_private_segment(m)
    _within_two_workgroups_per_cu(co)
    co3 = _co(tmp_path_factory, "lqr3", "cd_r12", ranks=(12,))
    m3 = _meta(co3)
    _expect_forms(_corr(m3, "8RtcModel"), (12,))
    _no_private_segment(m3)
    _within_two_workgroups_per_cu(co3)


def test_three_dimensional_corr_forms_have_no_private_segment_at_ranks_4_and_8(tmp_path_factory):
    """the two-pair model in three dimensions (a middle core in every point evaluation), with horizon and stop on top: no form
    at ranks 4 and 8 has a private segment, and none spills"""
    co = _co(tmp_path_factory, "lqr3", "cd_hs", ranks=(4, 8), horizon=True, stop=True)
    m = _meta(co)
    for inner in ("8RtcModel", "9HorizonOfINS_8RtcModel", "6StopOfINS_8RtcModel", "6StopOfINS_9HorizonOfINS_8RtcModel"):
        _expect_forms(_corr(m, inner), (4, 8))
    _no_private_segment(m)
    _within_two_workgroups_per_cu(co)


def _cd(spec, ncorr, dims=(), game=0, horizon=0, stop=0, njump=0, nimpulse=0):
    cd = E.ModelSpecCd(E.ModelSpecIc(E.ModelSpecJd(E.ModelSpecOs(E.ModelSpecFh(E.ModelSpecEx(spec, game), horizon), stop), njump), nimpulse), ncorr)
    for q, v in enumerate(dims):
        cd.corr_dims[q] = v
    return cd


@pytest.mark.parametrize("njump", [0, 3])
def test_spec_with_ncorr_0_yields_the_ic_code_object(tmp_path, njump):
    """... and needs no covar in the source"""
    src, masks = (JL.LQR, JL.LQR_MASKS)
    name = f"lqr_cd0_{njump}"
    ref = E.code_object(src, 2, 2, ranks=(4, 8), name=name, njump=njump, **masks)
    L = E.load_library()
    spec = E._model_spec(src, 2, 2, (4, 8), False, masks["udep_mask"], masks["uconst_mask"], True, name)
    cd = _cd(spec, 0, njump=njump)
    size = C.c_size_t(len(ref) + 1024)
    buf = C.create_string_buffer(size.value)
    assert L.c3sc_hip_model_code_object_cd(C.byref(cd), buf, C.byref(size)) == 0
    assert b"CorrOf" not in ref
    a, b = tmp_path / "ic.co", tmp_path / "cd.co"
    a.write_bytes(ref)
    b.write_bytes(buf.raw[:size.value])
    assert _meta(a) == _meta(b) and _bodies(a) == _bodies(b)  # equal metadata and equal bodies


def test_source_without_covar_compiles_only_with_ncorr_0():
    with pytest.raises(E.C3scHipError) as ei:
        E.compile_model(SL.LQR, 2, 2, ranks=(4,), name="lqr_nocovar", corr_pairs=[(0, 1)], **SL.LQR_MASKS)
    assert ei.value.args[1] == ERR_ARG
    assert "covar" in str(ei.value)


def test_bad_pair_lists_are_argument_errors():
    L = E.load_library()
    spec = E._model_spec(CL.LQR3, 3, 3, (4,), False, 0, 0, True, "lqr3_cd_bad")
    mid = C.c_int(0)
    bad = [(-1, ()), (9, tuple(range(16))), (100, ()), (1, (0, 3)), (1, (-1, 1)), (1, (1, 1)), (1, (2, 1)), (2, (0, 1, 0, 1)), (3, (0, 1, 1, 2, 0, 1))]
    for ncorr, dims in bad:
        cd = _cd(spec, ncorr, dims)
        assert L.c3sc_hip_model_compile_cd(C.byref(cd), C.byref(mid)) == ERR_ARG, (ncorr, dims)
        size = C.c_size_t(0)
        assert L.c3sc_hip_model_code_object_cd(C.byref(cd), None, C.byref(size)) == ERR_ARG, (ncorr, dims)
    assert L.c3sc_hip_model_compile_cd(None, C.byref(mid)) == ERR_ARG
    size = C.c_size_t(0)
    assert L.c3sc_hip_model_code_object_cd(None, None, C.byref(size)) == ERR_ARG
    with pytest.raises(E.C3scHipError) as ei:
        E.compile_model(CL.LQR3, 3, 3, ranks=(4,), corr_pairs=[(0, 1)] * 9, **CL.LQR3_MASKS)
    assert ei.value.args[1] == ERR_ARG
    with pytest.raises(E.C3scHipError) as ei:
        E.compile_model(CL.LQR, 2, 2, ranks=(4,), corr_pairs=[(0, 2)], **CL.LQR_MASKS)
    assert ei.value.args[1] == ERR_ARG


@pytest.mark.parametrize("kw", [dict(game=True), dict(box=True), dict(nimpulse=3)])
def test_pairs_with_game_box_or_interventions_are_refused(kw):
    src = IL.LQR + CL.LQR_COVAR if "nimpulse" in kw else CL.LQR
    with pytest.raises(E.C3scHipError) as ei:
        E.compile_model(src, 2, 2, ranks=(4,), corr_pairs=[(0, 1)], **kw)
    assert ei.value.args[1] == ERR_UNSUPPORTED


def test_library_kernels_have_no_corr_form(tmp_path):
    """the compiler's resource remarks of this build, regenerated from the *.res files: no library kernel is a corr
    instantiation, and the library still has its 666 entries"""
    import glob
    import json
    import shutil

    res = glob.glob(os.path.join(ROOT, "c3sc_amd", "csrc", "*.res"))
    assert res, "the build keeps the compiler's resource remarks next to the objects"
    for f in res:
        shutil.copy(f, tmp_path)
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), str(tmp_path)], check=True, capture_output=True)
    names = json.load(open(tmp_path / "kernel_resources.json"))
    assert len(names) == 666
    assert not any("CorrOf" in n for n in names)


def test_kargs_keeps_its_size(tmp_path):
    """whether a launch takes the corr form is host state (the FORM_CORR bit of LaunchIO::form): the kernels' argument block is the old one"""
    src = tmp_path / "kargs.hip"
    src.write_text('#include "kernel_common.hpp"\nstatic_assert(sizeof(c3sc::KArgs) == 1368);\nstruct M0 {};\n'
                   "static_assert(c3sc::model_corr<c3sc::CorrOf<c3sc::JumpOf<M0>>>());\n"
                   "static_assert(c3sc::model_jump<c3sc::CorrOf<c3sc::JumpOf<M0>>>());\n"
                   "static_assert(!c3sc::model_corr<c3sc::JumpOf<M0>>());\n")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    r = subprocess.run([hipcc, "-std=c++20", "-x", "hip", "--offload-arch=gfx950", "-fsyntax-only",
                        "-I", os.path.join(ROOT, "c3sc_amd", "csrc"), "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


def test_ctypes_spec_has_the_c_struct_layout(tmp_path):
    """engine.ModelSpecCd against struct c3sc_hip_model_spec_cd of include/c3sc_hip.h: size and offsets, checked by the C
    compiler"""
    src = tmp_path / "spec.c"
    src.write_text('#include <stddef.h>\n#include "c3sc_hip.h"\n'
                   f"_Static_assert(sizeof(c3sc_hip_model_spec_cd) == {C.sizeof(E.ModelSpecCd)}, \"size\");\n"
                   f"_Static_assert(offsetof(c3sc_hip_model_spec_cd, ncorr) == {E.ModelSpecCd.ncorr.offset}, \"ncorr\");\n"
                   f"_Static_assert(offsetof(c3sc_hip_model_spec_cd, corr_dims) == {E.ModelSpecCd.corr_dims.offset}, \"corr_dims\");\n"
                   f"_Static_assert(offsetof(c3sc_hip_model_spec_cd, ic.nimpulse) == {E.ModelSpecIc.nimpulse.offset}, \"nimpulse\");\n"
                   f"_Static_assert(C3SC_CORR_MAX == {E.CORR_MAX}, \"max\");\n"
                   "_Static_assert(C3SC_STATUS_DOMINANCE == 4, \"status\");\n")
    r = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
