"""Jump diffusions, compile side (c3sc_hip_model_compile_jd / c3sc_hip_model_code_object_jd): no GPU is needed.
The new symbols are exported; a jump model's code object is for gfx950 and holds the jump forms of the per-wave kernels the
other flags select (plain, horizon, stop, horizon with stop; at rank 12 the L2 form too) and of k_rollout next to the forms
without jumps, never a k_rollout_ode form, with the rollouts' cross-lane rule (tests/test_stop_build.py, restated);
njump = 0 yields the _os code object instruction for instruction and needs neither function in the source; njump outside
0..8 is an argument error, jumps with a game or the box are refused; the library itself holds no jump kernel."""
import ctypes as C
import os
import subprocess
import sys

import pytest

from c3sc_amd import engine as E
import jump_lib as JL
from test_rtc_model_build import CROSS_LANE, READELF, _bodies, _instr, _meta, _vregs

ERR_ARG, ERR_UNSUPPORTED = 1, 3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = {"lqr": (JL.LQR, 2, 2, JL.LQR_MASKS, JL.LQR_NJUMP), "put": (JL.PUT, 2, 1, JL.PUT_MASKS, JL.PUT_NJUMP),
          "lqr3": (JL.LQR3, 3, 3, JL.LQR3_MASKS, JL.LQR3_NJUMP)}


def _co(tmp_path_factory, model, tag, **kw):
    src, d, du, masks, nj = MODELS[model]
    co = E.code_object(src, d, du, name=f"{model}_{tag}", njump=nj, **masks, **kw)
    p = tmp_path_factory.mktemp("co") / f"{model}_{tag}.co"
    p.write_bytes(co)
    return p


def test_new_symbols_are_exported_with_plain_c_names():
    L = E.load_library()
    for n in ("c3sc_hip_model_compile_jd", "c3sc_hip_model_code_object_jd", "c3sc_hip_set_jumps"):
        assert hasattr(L, n), n
        assert n in E.EXPORTS, n
    assert E.JUMP_MAX == JL.JUMP_MAX == 8


def _jump(m, horizon, stop):
    """the jump kernels of the (horizon, stop) form: JumpOf wraps StopOf wraps HorizonOf wraps the model"""
    inner = "JumpOfINS_" + ("6StopOfINS_" if stop else "") + ("9HorizonOfINS_" if horizon else "") + "8RtcModel"
    return [k for k in m if inner in k]


def _check_lane_rule(co, expect):
    """the rollouts' lane rule of DESIGN.md 4.8 on the jump rollouts: global loads only, no cross-lane operation, v_readlane of
    SGPR spill slots alone"""
    seen = 0
    for name, body in _bodies(co).items():
        if "k_rollout" not in name or "JumpOf" not in name:
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
    assert seen == expect, (seen, expect)


def _expect_forms(names, ranks):
    for rp in ranks:
        for npl in (1, 2):
            for staged in ((1,) if rp < 12 else (0, 1)):
                n = sum("k_fiber_per_wave" in k and f"ELi{rp}ELi{npl}ELb0ELb0ELb{staged}E" in k for k in names)
                assert n == 1, (rp, npl, staged, n)
        assert sum("k_rolloutI" in k and f"ELi{rp}ELb0E" in k for k in names) == 1, rp
    assert not any("k_rollout_ode" in k for k in names), "integrate has no jump form"
    assert len(names) == sum((2 if rp < 12 else 4) + 1 for rp in ranks), names


@pytest.mark.parametrize("horizon", [False, True], ids=["infinite", "horizon"])
@pytest.mark.parametrize("stop", [False, True], ids=["nostop", "stop"])
def test_jump_code_object_holds_the_jump_forms_of_every_flag_combination(tmp_path_factory, horizon, stop):
    for model in ("lqr", "put"):
        co = _co(tmp_path_factory, model, f"jd_{int(horizon)}{int(stop)}", ranks=(4, 8), horizon=horizon, stop=stop)
        hdr = subprocess.run([READELF, "-h", str(co)], check=True, capture_output=True, text=True).stdout
        assert "EM_AMDGPU" in hdr and "gfx950" in hdr
        m = _meta(co)
        total = 0
        for hz in (False, True):
            for sp in (False, True):
                names = _jump(m, hz, sp)
                if (hz and not horizon) or (sp and not stop):
                    assert not names, (hz, sp, names)
                else:
                    _expect_forms(names, (4, 8))
                    total += len(names)
        assert len([k for k in m if "JumpOf" in k]) == total
        _check_lane_rule(co, 2 * (1 + int(horizon)) * (1 + int(stop)))
        assert len([k for k in m if "RtcModel" in k and "JumpOf" not in k and "StopOf" not in k and "HorizonOf" not in k]) == 2 * 4
        for name, priv in m.items():
            assert priv == 0, f"{name}: private segment of {priv} bytes at ranks 4 and 8"


def test_jump_forms_at_rank_12_include_the_l2_per_wave_kernel(tmp_path_factory):
    for model in ("lqr", "lqr3"):
        m = _meta(_co(tmp_path_factory, model, "jd_r12", ranks=(12,), horizon=True, stop=True))
        for hz in (False, True):
            for sp in (False, True):
                _expect_forms(_jump(m, hz, sp), (12,))


@pytest.mark.parametrize("horizon,stop", [(0, 0), (1, 0), (1, 1)])
def test_spec_with_njump_0_yields_the_os_code_object(tmp_path, horizon, stop):
    """... and needs neither jumprate nor jump in the source"""
    import stop_lib as SL

    src, masks = SL.LQR, SL.LQR_MASKS
    name = f"lqr_jd0_{horizon}{stop}"
    ref = E.code_object(src, 2, 2, ranks=(4, 8), name=name, horizon=bool(horizon), stop=bool(stop), **masks)
    L = E.load_library()
    spec = E._model_spec(src, 2, 2, (4, 8), False, masks["udep_mask"], masks["uconst_mask"], True, name)
    jd = E.ModelSpecJd(E.ModelSpecOs(E.ModelSpecFh(E.ModelSpecEx(spec, 0), horizon), stop), 0)
    size = C.c_size_t(len(ref) + 1024)
    buf = C.create_string_buffer(size.value)
    assert L.c3sc_hip_model_code_object_jd(C.byref(jd), buf, C.byref(size)) == 0
    assert b"JumpOf" not in ref
    a, b = tmp_path / "os.co", tmp_path / "jd.co"
    a.write_bytes(ref)
    b.write_bytes(buf.raw[:size.value])
    assert _meta(a) == _meta(b) and _bodies(a) == _bodies(b)  # equal metadata and equal bodies


def test_source_without_the_jump_functions_compiles_only_with_njump_0():
    import stop_lib as SL

    with pytest.raises(E.C3scHipError) as ei:
        E.compile_model(SL.LQR, 2, 2, ranks=(4,), name="lqr_nojumpfn", njump=2, **SL.LQR_MASKS)
    assert ei.value.args[1] == ERR_ARG
    assert "jump" in str(ei.value)


def test_njump_out_of_range_is_an_argument_error():
    L = E.load_library()
    spec = E._model_spec(JL.LQR, 2, 2, (4,), False, 0, 0, True, "lqr_jd_bad")
    mid = C.c_int(0)
    for nj in (-1, 9, 100):
        jd = E.ModelSpecJd(E.ModelSpecOs(E.ModelSpecFh(E.ModelSpecEx(spec, 0), 0), 0), nj)
        assert L.c3sc_hip_model_compile_jd(C.byref(jd), C.byref(mid)) == ERR_ARG
        size = C.c_size_t(0)
        assert L.c3sc_hip_model_code_object_jd(C.byref(jd), None, C.byref(size)) == ERR_ARG
    assert L.c3sc_hip_model_compile_jd(None, C.byref(mid)) == ERR_ARG
    size = C.c_size_t(0)
    assert L.c3sc_hip_model_code_object_jd(None, None, C.byref(size)) == ERR_ARG
    with pytest.raises(E.C3scHipError) as ei:
        E.compile_model(JL.LQR, 2, 2, ranks=(4,), njump=9, **JL.LQR_MASKS)
    assert ei.value.args[1] == ERR_ARG


@pytest.mark.parametrize("kw", [dict(game=True), dict(box=True)])
def test_jumps_with_game_or_box_are_refused(kw):
    with pytest.raises(E.C3scHipError) as ei:
        E.compile_model(JL.LQR, 2, 2, ranks=(4,), njump=3, **kw)
    assert ei.value.args[1] == ERR_UNSUPPORTED


def test_a_model_with_eight_marks_compiles(tmp_path):
    src = JL.KNOWN.replace("m == 2 ? 0.5 : 0.25", "0.125")
    co = E.code_object(src, 2, 1, ranks=(4,), name="known8", njump=8, **JL.KNOWN_MASKS)
    p = tmp_path / "k8.co"
    p.write_bytes(co)
    assert len([k for k in _meta(p) if "JumpOf" in k]) == 3


def test_library_kernels_have_no_jump_form(tmp_path):
    """the compiler's resource remarks of this build, regenerated from the *.res files: no library kernel is a jump
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
    assert not any("JumpOf" in n for n in names)
