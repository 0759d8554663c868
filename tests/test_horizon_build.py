"""Finite-horizon problems, compile side (c3sc_hip_model_compile_fh / c3sc_hip_model_code_object_fh): no GPU is
needed.  The new symbols are exported; a horizon model's code object is for gfx950 and holds the horizon forms of the per-wave
and rollout kernels next to the plain ones, without scratch at ranks 4 and 8, with the rollouts' cross-lane rule
(tests/test_rtc_model_build.py, restated for the horizon kernels); a spec without the flag yields the kernels it always did; the
library itself holds no horizon kernel and KArgs keeps its size and offsets; horizon with game or box is refused."""
import ctypes as C
import os
import subprocess
import sys

import pytest

from c3sc_amd import engine as E
from horizon_lib import LQR, LQR_MASKS, PENDULUM, PENDULUM_MASKS
from test_rtc_model_build import CROSS_LANE, _bodies, _instr, _meta, _vregs

ERR_ARG, ERR_UNSUPPORTED = 1, 3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lqr_co(tmp_path_factory):
    co = E.code_object(LQR, 2, 2, ranks=(4, 8), name="lqr_fh_co", horizon=True, **LQR_MASKS)
    p = tmp_path_factory.mktemp("co") / "lqr.co"
    p.write_bytes(co)
    return p


@pytest.fixture(scope="module")
def pendulum_co(tmp_path_factory):
    co = E.code_object(PENDULUM, 2, 2, ranks=(4, 8), name="pendulum_fh_co", horizon=True, **PENDULUM_MASKS)
    p = tmp_path_factory.mktemp("co") / "pendulum.co"
    p.write_bytes(co)
    return p


def test_new_symbols_are_exported_with_plain_c_names():
    L = E.load_library()
    for n in ("c3sc_hip_model_compile_fh", "c3sc_hip_model_code_object_fh", "c3sc_hip_set_horizon_step",
              "c3sc_hip_upload_value_stack"):
        assert hasattr(L, n), n
        assert n in E.EXPORTS, n
    H = C.CDLL(E.LIB_PATH.replace("csrc/libc3sc_hip.so", "host/libc3sc.so"))
    for n in ("c3control_set_horizon_step", "c3control_get_horizon_step", "c3control_fh_solve"):
        assert hasattr(H, n), n


def test_horizon_code_object_is_gfx950_and_holds_the_horizon_kernels(lqr_co, pendulum_co):
    from test_rtc_model_build import READELF
    hdr = subprocess.run([READELF, "-h", str(lqr_co)], check=True, capture_output=True, text=True).stdout
    assert "EM_AMDGPU" in hdr and "gfx950" in hdr
    for co in (lqr_co, pendulum_co):
        m = _meta(co)
        hz = [k for k in m if "HorizonOf" in k]
        for rp in (4, 8):
            for npl in (1, 2):
                assert sum("k_fiber_per_wave" in k and f"EEEELi{rp}ELi{npl}ELb0ELb0ELb1E" in k for k in hz) == 1, (rp, npl)
            assert sum("k_rolloutI" in k and f"EEEELi{rp}ELb0E" in k for k in hz) == 1, rp
            assert not any("k_rollout_ode" in k for k in hz), "integrate has no horizon form"
        assert len(hz) == 2 * 3
        assert len([k for k in m if "RtcModel" in k and "HorizonOf" not in k]) == 2 * 4  # the plain forms stay


def test_horizon_forms_at_rank_12_include_the_l2_per_wave_kernel(tmp_path):
    co = E.code_object(LQR, 2, 2, ranks=(12,), name="lqr_fh_r12", horizon=True, **LQR_MASKS)
    p = tmp_path / "r12.co"
    p.write_bytes(co)
    hz = [k for k in _meta(p) if "HorizonOf" in k]
    for npl in (1, 2):
        for staged in (0, 1):
            assert sum("k_fiber_per_wave" in k and f"EEEELi12ELi{npl}ELb0ELb0ELb{staged}E" in k for k in hz) == 1, (npl, staged)
    assert sum("k_rolloutI" in k for k in hz) == 1


def test_no_scratch_at_ranks_4_and_8(lqr_co, pendulum_co):
    for co in (lqr_co, pendulum_co):
        for name, priv in _meta(co).items():
            assert priv == 0, f"{name}: private segment of {priv} bytes"


def test_horizon_rollouts_keep_the_cross_lane_rule(lqr_co, pendulum_co):
    seen = 0
    for co in (lqr_co, pendulum_co):
        for name, body in _bodies(co).items():
            if "k_rollout" not in name or "HorizonOf" not in name:
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
    assert seen == 2 * 2


def test_spec_without_horizon_yields_the_kernels_it_always_did(tmp_path):
    plain = E.code_object(LQR, 2, 2, ranks=(4, 8), name="lqr_plain", **LQR_MASKS)
    L = E.load_library()
    spec = E._model_spec(LQR, 2, 2, (4, 8), False, LQR_MASKS["udep_mask"], LQR_MASKS["uconst_mask"], True, "lqr_plain")
    fh = E.ModelSpecFh(E.ModelSpecEx(spec, 0), 0)
    size = C.c_size_t(len(plain) + 1024)
    buf = C.create_string_buffer(size.value)
    assert L.c3sc_hip_model_code_object_fh(C.byref(fh), buf, C.byref(size)) == 0
    assert b"HorizonOf" not in plain
    a, b = tmp_path / "plain.co", tmp_path / "fh.co"
    a.write_bytes(plain)
    b.write_bytes(buf.raw[:size.value])
    assert _meta(a) == _meta(b) and _bodies(a) == _bodies(b)  # the same kernels, instruction for instruction


def test_library_kernels_have_no_horizon_form(tmp_path):
    """the compiler's resource remarks of this build (regenerated from the *.res files, not an older kernel_resources.json): no
    library kernel is a horizon instantiation, so the library's kernels are the ones the plain templates always produced"""
    import glob
    import json
    import shutil

    res = glob.glob(os.path.join(ROOT, "c3sc_amd", "csrc", "*.res"))
    assert res, "the build keeps the compiler's resource remarks next to the objects"
    for f in res:
        shutil.copy(f, tmp_path)
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), str(tmp_path)], check=True, capture_output=True)
    names = json.load(open(tmp_path / "kernel_resources.json"))
    assert names and not any("HorizonOf" in n for n in names)
    assert any(n.startswith("k_fiber_per_wave<") for n in names)


def test_kargs_keeps_its_size_and_offsets(tmp_path):
    """the horizon offset sits in the alignment hole after tbl_off: the size and the neighbours' offsets are the old ones"""
    src = tmp_path / "kargs.hip"
    src.write_text('#include "kernel_common.hpp"\n#include <cstddef>\nusing c3sc::KArgs;\n'
                   "static_assert(sizeof(KArgs) == 1368);\n"
                   "static_assert(offsetof(KArgs, tbl_off) == 688 && offsetof(KArgs, hz_off) == 692);\n"
                   "static_assert(offsetof(KArgs, quad_coreT_off) == 696 && offsetof(KArgs, cends) == 1192);\n"
                   "static_assert(offsetof(KArgs, game_gsz) == 1196 && offsetof(KArgs, img_base) == 1360);\n")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    r = subprocess.run([hipcc, "-std=c++20", "-x", "hip", "--offload-arch=gfx950", "-fsyntax-only",
                        "-I", os.path.join(ROOT, "c3sc_amd", "csrc"), "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


@pytest.mark.parametrize("kw,code", [(dict(game=True), ERR_UNSUPPORTED), (dict(box=True), ERR_UNSUPPORTED)])
def test_horizon_with_game_or_box_is_refused(kw, code):
    with pytest.raises(E.C3scHipError) as ei:
        E.compile_model(LQR, 2, 2, ranks=(4,), horizon=True, **kw)
    assert ei.value.args[1] == code


def test_bad_horizon_flag_is_refused():
    L = E.load_library()
    spec = E._model_spec(LQR, 2, 2, (4,), False, 0, 0, True, "lqr_bad")
    fh = E.ModelSpecFh(E.ModelSpecEx(spec, 0), 2)
    mid = C.c_int(0)
    assert L.c3sc_hip_model_compile_fh(C.byref(fh), C.byref(mid)) == ERR_ARG
    assert L.c3sc_hip_model_compile_fh(None, C.byref(mid)) == ERR_ARG
