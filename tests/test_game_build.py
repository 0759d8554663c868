"""Zero-sum games, compile side (c3sc_hip_model_compile_ex / c3sc_hip_model_code_object_ex): no GPU is needed.
The new symbols are exported; a game model's code object is for gfx950 and holds the game forms of the per-wave, rollout and
integrate kernels next to the plain ones, without scratch at ranks 4 and 8, with the rollouts' cross-lane rule
(tests/test_rtc_model_build.py, restated for the game kernels); a spec compiled without the game flag yields the kernels it
always did; bad game specs are refused."""
import ctypes as C

import pytest

from c3sc_amd import engine as E
from game_lib import LQGAME, LQGAME_MASKS, PURSUIT, PURSUIT_MASKS
from test_rtc_model_build import CROSS_LANE, _bodies, _instr, _meta, _vregs

ERR_ARG, ERR_UNSUPPORTED = 1, 3


@pytest.fixture(scope="module")
def game_co(tmp_path_factory):
    co = E.code_object(LQGAME, 2, 2, ranks=(4, 8), name="lqgame_co", game=True, **LQGAME_MASKS)
    p = tmp_path_factory.mktemp("co") / "lqgame.co"
    p.write_bytes(co)
    return p


@pytest.fixture(scope="module")
def pursuit_co(tmp_path_factory):
    co = E.code_object(PURSUIT, 3, 2, ranks=(4, 8), name="pursuit_co", game=True, **PURSUIT_MASKS)
    p = tmp_path_factory.mktemp("co") / "pursuit.co"
    p.write_bytes(co)
    return p


def test_new_symbols_are_exported_with_plain_c_names():
    L = E.load_library()
    for n in ("c3sc_hip_set_game", "c3sc_hip_model_compile_ex", "c3sc_hip_model_code_object_ex"):
        assert hasattr(L, n), n
    H = C.CDLL(E.LIB_PATH.replace("csrc/libc3sc_hip.so", "host/libc3sc.so"))
    for n in ("c3opt_set_brute_force_game", "c3opt_get_game"):
        assert hasattr(H, n), n


def test_game_code_object_is_gfx950_and_holds_the_game_kernels(game_co, pursuit_co):
    import subprocess
    from test_rtc_model_build import READELF
    hdr = subprocess.run([READELF, "-h", str(game_co)], check=True, capture_output=True, text=True).stdout
    assert "EM_AMDGPU" in hdr and "gfx950" in hdr
    for co in (game_co, pursuit_co):
        m = _meta(co)
        game = [k for k in m if "GameOf" in k]
        for rp in (4, 8):
            for npl in (1, 2):
                assert sum("k_fiber_per_wave" in k and f"EEEELi{rp}ELi{npl}ELb0ELb0ELb1E" in k for k in game) == 1, (rp, npl)
            assert sum("k_rolloutI" in k and f"EEEELi{rp}ELb0E" in k for k in game) == 1, rp
            assert sum("k_rollout_ode" in k and f"EEEELi{rp}ELb0E" in k for k in game) == 1, rp
        assert len(game) == 2 * 4
        assert len([k for k in m if "RtcModel" in k and "GameOf" not in k]) == 2 * 4  # the plain forms stay


def test_no_scratch_at_ranks_4_and_8(game_co, pursuit_co):
    for co in (game_co, pursuit_co):
        for name, priv in _meta(co).items():
            assert priv == 0, f"{name}: private segment of {priv} bytes"


def test_game_rollouts_keep_the_cross_lane_rule(game_co, pursuit_co):
    seen = 0
    for co in (game_co, pursuit_co):
        for name, body in _bodies(co).items():
            if "k_rollout" not in name or "GameOf" not in name:
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
    assert seen == 2 * 2 * 2


def test_spec_without_game_yields_the_kernels_it_always_did(tmp_path):
    plain = E.code_object(LQGAME, 2, 2, ranks=(4, 8), name="lqgame_plain", **LQGAME_MASKS)
    L = E.load_library()
    spec = E._model_spec(LQGAME, 2, 2, (4, 8), False, LQGAME_MASKS["udep_mask"], LQGAME_MASKS["uconst_mask"], True, "lqgame_plain")
    ex = E.ModelSpecEx(spec, 0)
    size = C.c_size_t(len(plain) + 1024)
    buf = C.create_string_buffer(size.value)
    assert L.c3sc_hip_model_code_object_ex(C.byref(ex), buf, C.byref(size)) == 0
    assert b"GameOf" not in plain
    a, b = tmp_path / "plain.co", tmp_path / "ex.co"
    a.write_bytes(plain)
    b.write_bytes(buf.raw[:size.value])
    assert _meta(a) == _meta(b) and _bodies(a) == _bodies(b)  # the same kernels, instruction for instruction


@pytest.mark.parametrize("kw,code", [(dict(du=1), ERR_ARG), (dict(box=True), ERR_UNSUPPORTED)])
def test_bad_game_specs_are_refused(kw, code):
    args = dict(d=2, du=2, ranks=(4,), game=True)
    args.update(kw)
    with pytest.raises(E.C3scHipError) as ei:
        E.compile_model(LQGAME if args["du"] == 2 else LQGAME.replace("u[1]", "0.0"), **args)
    assert ei.value.args[1] == code


def test_game_split():
    assert E.game_split(7, 3) == (2, 1)
    assert E.game_split(-1, 3) == (-1, -1)
    iu, iw = E.game_split([0, 5, -1], 3)
    assert list(iu) == [0, 1, -1] and list(iw) == [0, 2, -1]
