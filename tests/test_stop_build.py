"""Optimal stopping, compile side (c3sc_hip_model_compile_os / c3sc_hip_model_code_object_os): no GPU is needed.
The new symbols are exported; a stopping model's code object is for gfx950 and holds the stop forms of the per-wave and rollout
kernels next to the plain ones (with horizon = 1 the combined forms too, at rank 12 the L2 per-wave form, never a
k_rollout_ode form), without scratch at ranks 4 and 8 and with the rollouts' cross-lane rule (tests/test_horizon_build.py,
restated for the stop kernels); a spec with stop = 0 yields the _fh code object's kernels; stop with game or box is refused; a
source without stopcost compiles unless the flag is set; the library itself holds no stop kernel and KArgs keeps its size."""
import ctypes as C
import os
import subprocess
import sys

import pytest

from c3sc_amd import engine as E
import stop_lib as SL
from test_rtc_model_build import CROSS_LANE, READELF, _bodies, _instr, _meta, _vregs

ERR_ARG, ERR_UNSUPPORTED = 1, 3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = {"lqr": (SL.LQR, 2, SL.LQR_MASKS), "put": (SL.PUT, 1, SL.PUT_MASKS)}


def _co(tmp_path_factory, model, tag, **kw):
    src, du, masks = MODELS[model]
    co = E.code_object(src, 2, du, name=f"{model}_{tag}", stop=True, **masks, **kw)
    p = tmp_path_factory.mktemp("co") / f"{model}_{tag}.co"
    p.write_bytes(co)
    return p


@pytest.fixture(scope="module")
def stop_cos(tmp_path_factory):
    return [_co(tmp_path_factory, m, "os_co", ranks=(4, 8)) for m in MODELS]


@pytest.fixture(scope="module")
def american_cos(tmp_path_factory):
    return [_co(tmp_path_factory, m, "am_co", ranks=(4, 8), horizon=True) for m in MODELS]


def test_new_symbols_are_exported_with_plain_c_names():
    L = E.load_library()
    for n in ("c3sc_hip_model_compile_os", "c3sc_hip_model_code_object_os", "c3sc_hip_set_stopping"):
        assert hasattr(L, n), n
        assert n in E.EXPORTS, n
    H = C.CDLL(E.LIB_PATH.replace("csrc/libc3sc_hip.so", "host/libc3sc.so"))
    for n in ("c3control_add_stopcost", "c3control_set_stopping", "c3control_get_stopping", "c3control_policy_eval_stop"):
        assert hasattr(H, n), n


def _stop_only(m):
    return [k for k in m if "StopOf" in k and "HorizonOf" not in k]


def _american(m):
    return [k for k in m if "StopOfINS_9HorizonOf" in k]


def _expect_forms(names, ranks):
    for rp in ranks:
        for npl in (1, 2):
            for staged in ((1,) if rp < 12 else (0, 1)):
                n = sum("k_fiber_per_wave" in k and f"ELi{rp}ELi{npl}ELb0ELb0ELb{staged}E" in k for k in names)
                assert n == 1, (rp, npl, staged, n)
        assert sum("k_rolloutI" in k and f"ELi{rp}ELb0E" in k for k in names) == 1, rp
    assert not any("k_rollout_ode" in k for k in names), "integrate has no stop form"
    assert len(names) == sum((2 if rp < 12 else 4) + 1 for rp in ranks)


def test_stop_code_object_is_gfx950_and_holds_the_stop_kernels(stop_cos):
    hdr = subprocess.run([READELF, "-h", str(stop_cos[0])], check=True, capture_output=True, text=True).stdout
    assert "EM_AMDGPU" in hdr and "gfx950" in hdr
    for co in stop_cos:
        m = _meta(co)
        _expect_forms(_stop_only(m), (4, 8))
        assert not any("HorizonOf" in k for k in m)
        assert len([k for k in m if "RtcModel" in k and "StopOf" not in k]) == 2 * 4  # the plain forms stay


def test_american_code_object_holds_the_stop_horizon_and_combined_kernels(american_cos):
    for co in american_cos:
        m = _meta(co)
        _expect_forms(_stop_only(m), (4, 8))
        _expect_forms(_american(m), (4, 8))
        _expect_forms([k for k in m if "HorizonOf" in k and "StopOf" not in k], (4, 8))
        assert len([k for k in m if "StopOf" in k]) == len(_stop_only(m)) + len(_american(m))
        assert not any("k_rollout_ode" in k and ("StopOf" in k or "HorizonOf" in k) for k in m)


def test_stop_forms_at_rank_12_include_the_l2_per_wave_kernel(tmp_path_factory):
    for model in MODELS:
        m = _meta(_co(tmp_path_factory, model, "os_r12", ranks=(12,), horizon=True))
        _expect_forms(_stop_only(m), (12,))
        _expect_forms(_american(m), (12,))


def test_no_scratch_at_ranks_4_and_8(stop_cos, american_cos):
    for co in stop_cos + american_cos:
        for name, priv in _meta(co).items():
            assert priv == 0, f"{name}: private segment of {priv} bytes"


def test_stop_rollouts_keep_the_cross_lane_rule(stop_cos, american_cos):
    seen = 0
    for co in stop_cos + american_cos:
        for name, body in _bodies(co).items():
            if "k_rollout" not in name or "StopOf" not in name:
                continue
            seen += 1
            assert not any("flat_load" in l for l in body), f"{name}: FLAT loads"
            slots = set()
            for l in body:
                op, args = _instr(l)
                if op and op.startswith("v_readlane"):
                    slots |= _vregs(args[1])
                assert not (op and CROSS_LANE.search(l)), f"{name}: cross-lane operation {l}"
            for l in body:
                op, args = _instr(l)
                if not op or op.startswith(("v_writelane", "v_readlane", "v_cmp", "v_readfirstlane")) or "store" in op or not args:
                    continue
                assert not (_vregs(args[0]) & slots), f"{name}: {l} writes a VGPR that v_readlane reads"
    assert seen == 2 * 2 + 2 * 4


@pytest.mark.parametrize("horizon", [0, 1])
def test_spec_with_stop_0_yields_the_fh_code_object(tmp_path, horizon):
    src, du, masks = MODELS["lqr"]
    name = f"lqr_os0_{horizon}"
    ref = E.code_object(src, 2, du, ranks=(4, 8), name=name, horizon=bool(horizon), **masks)
    L = E.load_library()
    spec = E._model_spec(src, 2, du, (4, 8), False, masks["udep_mask"], masks["uconst_mask"], True, name)
    os_ = E.ModelSpecOs(E.ModelSpecFh(E.ModelSpecEx(spec, 0), horizon), 0)
    size = C.c_size_t(len(ref) + 1024)
    buf = C.create_string_buffer(size.value)
    assert L.c3sc_hip_model_code_object_os(C.byref(os_), buf, C.byref(size)) == 0
    assert b"StopOf" not in ref
    a, b = tmp_path / "fh.co", tmp_path / "os.co"
    a.write_bytes(ref)
    b.write_bytes(buf.raw[:size.value])
    assert _meta(a) == _meta(b) and _bodies(a) == _bodies(b)  # equal metadata and equal bodies


def test_source_without_stopcost_compiles_only_without_the_flag():
    from horizon_lib import LQR, LQR_MASKS

    L = E.load_library()
    spec = E._model_spec(LQR, 2, 2, (4,), False, LQR_MASKS["udep_mask"], LQR_MASKS["uconst_mask"], True, "lqr_nostopcost")
    os_ = E.ModelSpecOs(E.ModelSpecFh(E.ModelSpecEx(spec, 0), 0), 0)
    size = C.c_size_t(0)
    assert L.c3sc_hip_model_code_object_os(C.byref(os_), None, C.byref(size)) == 0 and size.value > 0
    with pytest.raises(E.C3scHipError) as ei:
        E.compile_model(LQR, 2, 2, ranks=(4,), name="lqr_nostopcost", stop=True, **LQR_MASKS)
    assert ei.value.args[1] == ERR_ARG
    assert "stopcost" in str(ei.value)


@pytest.mark.parametrize("kw", [dict(game=True), dict(box=True), dict(game=True, horizon=True)])
def test_stop_with_game_or_box_is_refused(kw):
    with pytest.raises(E.C3scHipError) as ei:
        E.compile_model(SL.LQR, 2, 2, ranks=(4,), stop=True, **kw)
    assert ei.value.args[1] == ERR_UNSUPPORTED


def test_bad_stop_flag_is_refused():
    L = E.load_library()
    spec = E._model_spec(SL.LQR, 2, 2, (4,), False, 0, 0, True, "lqr_os_bad")
    mid = C.c_int(0)
    for flag in (2, -1):
        os_ = E.ModelSpecOs(E.ModelSpecFh(E.ModelSpecEx(spec, 0), 0), flag)
        assert L.c3sc_hip_model_compile_os(C.byref(os_), C.byref(mid)) == ERR_ARG
    assert L.c3sc_hip_model_compile_os(None, C.byref(mid)) == ERR_ARG
    size = C.c_size_t(0)
    assert L.c3sc_hip_model_code_object_os(None, None, C.byref(size)) == ERR_ARG


def test_library_kernels_have_no_stop_form(tmp_path):
    """the compiler's resource remarks of this build, regenerated from the *.res files: no library kernel is a stop
    instantiation"""
    import glob
    import json
    import shutil

    res = glob.glob(os.path.join(ROOT, "c3sc_amd", "csrc", "*.res"))
    assert res, "the build keeps the compiler's resource remarks next to the objects"
    for f in res:
        shutil.copy(f, tmp_path)
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), str(tmp_path)], check=True, capture_output=True)
    names = json.load(open(tmp_path / "kernel_resources.json"))
    assert names and not any("StopOf" in n for n in names)
    assert any(n.startswith("k_fiber_per_wave<") for n in names)


def test_decode_exit():
    import numpy as np

    step, stopped = E.decode_exit(np.array([-1, 0, 7, -2, -9]))
    assert step.tolist() == [-1, 0, 7, 0, 7] and stopped.tolist() == [0, 0, 0, 1, 1]
    assert E.decode_exit(-5) == (3, 1) and E.decode_exit(4) == (4, 0) and E.decode_exit(-1) == (-1, 0)
