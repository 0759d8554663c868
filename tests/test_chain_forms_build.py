"""The chain flag of the run-time model compiler (c3sc_hip_model_compile_mc) without a GPU: the new entry points
are exported and declared, the headers compile as C with C3SC_CHAIN_STOPPED, form_offered(., FORM_CHAIN) accepts exactly the eight
subsets of {horizon, stop, jump}, a chain = 1 code object holds exactly the walk and outcomes kernels of its forms, chain = 0 is
the _cd code object, and bad flag values are argument errors."""
import ctypes as C
import os
import re
import subprocess

import pytest

from c3sc_amd import engine as E
import jump_lib as JL
from test_rtc_model_build import READELF, _bodies, _meta

ERR_ARG = 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, S, J = 2, 4, 8  # FORM_HORIZON, FORM_STOP, FORM_JUMP
CHAIN = [0, H, S, H | S, J, H | J, S | J, H | S | J]  # written out, not computed from the rule
NEW = ("c3sc_hip_model_compile_mc", "c3sc_hip_model_code_object_mc", "c3sc_hip_chain_outcomes", "c3sc_hip_chain_outcomes_host")


def test_new_symbols_are_exported_and_declared():
    L = E.load_library()
    hdr = open(os.path.join(ROOT, "include", "c3sc_hip.h")).read()
    for n in NEW:
        assert hasattr(L, n), n
        assert n in E.EXPORTS, n
        assert re.search(r"^int " + n + r"\(", hdr, re.M), n
    assert "c3sc_hip_model_spec_mc" in hdr


def test_headers_compile_as_c99_with_the_stopped_word(tmp_path):
    src = tmp_path / "mc.c"
    src.write_text('#include <stddef.h>\n#include "c3sc_hip.h"\n'
                   f"_Static_assert(sizeof(c3sc_hip_model_spec_mc) == {C.sizeof(E.ModelSpecMc)}, \"size\");\n"
                   f"_Static_assert(offsetof(c3sc_hip_model_spec_mc, chain) == {E.ModelSpecMc.chain.offset}, \"chain\");\n"
                   f"_Static_assert(offsetof(c3sc_hip_model_spec_mc, cd.ncorr) == {E.ModelSpecCd.ncorr.offset}, \"ncorr\");\n"
                   "_Static_assert(C3SC_CHAIN_STOPPED(0) == -4294967298LL, \"step 0\");\n"
                   "_Static_assert(C3SC_CHAIN_STOPPED(5) == -7LL - 4294967296LL, \"step 5\");\n"
                   # disjoint from the stuck words of every call: nsteps <= 2^30
                   "_Static_assert(C3SC_CHAIN_STOPPED(0) < C3SC_CHAIN_STUCK(1073741824LL), \"disjoint\");\n"
                   "_Static_assert(C3SC_CHAIN_STUCK(3) == -5, \"stuck\");\n"
                   "int main(void) { int64_t e = C3SC_CHAIN_STOPPED(7); return e < 0 ? 0 : 1; }\n")
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert E.decode_chain_exit(-(7 + 2) - (1 << 32)) == (7, "stopped") and E.decode_chain_exit(-9) == (7, "stuck")
    assert E.decode_chain_exit(4) == (4, "exit") and E.decode_chain_exit(-1) == (-1, "running")


def test_the_rule_offers_the_chain_exactly_eight_forms(tmp_path):
    assert len(set(CHAIN)) == 8
    src = tmp_path / "chain_rule.hip"
    src.write_text('#include "kernel_common.hpp"\n'
                   + "".join(f"static_assert({'' if m in CHAIN else '!'}c3sc::form_offered({m}u, c3sc::FORM_CHAIN), \"FORM_CHAIN {m}\");\n"
                             for m in range(64))
                   + "static_assert(!c3sc::form_offered(64u, c3sc::FORM_CHAIN) && !c3sc::form_offered(~0u, c3sc::FORM_CHAIN));\n"
                   "static_assert(c3sc::FORM_CHAIN == c3sc::FORM_BOX + 1);\n"
                   "static_assert(sizeof(c3sc::KArgs) == 1368);\n")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    r = subprocess.run([hipcc, "-std=c++20", "-x", "hip", "--offload-arch=gfx950", "-fsyntax-only",
                        "-I", os.path.join(ROOT, "c3sc_amd", "csrc"), "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


KW = dict(horizon=True, stop=True, njump=JL.LQR_NJUMP, **JL.LQR_MASKS)


def test_chain_code_object_holds_the_kernels_of_the_eight_forms(tmp_path):
    co = E.code_object(JL.LQR, 2, 2, ranks=(4,), name="lqr_mc_hsj", chain=True, **KW)
    p = tmp_path / "mc.co"
    p.write_bytes(co)
    hdr = subprocess.run([READELF, "-h", str(p)], check=True, capture_output=True, text=True).stdout
    assert "EM_AMDGPU" in hdr and "gfx950" in hdr
    m = _meta(p)
    for kern in ("k_chain_walk_form", "k_chain_outcomes_form"):
        names = [k for k in m if kern in k]
        # <MID, RtcModel<..>, 4, FORM>: the last two template arguments in the mangled name
        forms = sorted(int(re.search(r"ELi4ELj(\d+)EE", k).group(1)) for k in names)
        assert forms == sorted(CHAIN), (kern, forms)
    assert not any(("k_chain_walk" in k or "k_chain_transitions" in k or "k_chain_outcomes" in k) and "_form" not in k for k in m)
    # ... beside the kernels the same spec has without the flag
    q = tmp_path / "cd.co"
    q.write_bytes(E.code_object(JL.LQR, 2, 2, ranks=(4,), name="lqr_mc_hsj", **KW))
    plain = _meta(q)
    assert not any("k_chain" in k for k in plain)
    assert sorted(k for k in m if "k_chain" not in k) == sorted(plain)
    # a jump-only spec: the plain form and the jump form
    r = tmp_path / "j.co"
    r.write_bytes(E.code_object(JL.LQR, 2, 2, ranks=(4,), name="lqr_mc_j", njump=JL.LQR_NJUMP, chain=True, **JL.LQR_MASKS))
    mj = _meta(r)
    assert sorted(int(re.search(r"ELi4ELj(\d+)EE", k).group(1)) for k in mj if "k_chain_walk_form" in k) == [0, J]


def _mc(chain, name):
    spec = E._model_spec(JL.LQR, 2, 2, (4,), False, JL.LQR_MASKS["udep_mask"], JL.LQR_MASKS["uconst_mask"], JL.LQR_MASKS["stage_udep"], name)
    mc, suffix = E._form_spec(spec, False, True, True, JL.LQR_NJUMP, 0, (), chain=1)
    assert suffix == "_mc" and isinstance(mc, E.ModelSpecMc)
    mc.chain = chain
    mc._keep = spec
    return mc


def test_chain_0_is_the_cd_code_object(tmp_path):
    L = E.load_library()
    ref = E.code_object(JL.LQR, 2, 2, ranks=(4,), name="lqr_mc0", **KW)
    mc = _mc(0, "lqr_mc0")
    size = C.c_size_t(len(ref) + 1024)
    buf = C.create_string_buffer(size.value)
    assert L.c3sc_hip_model_code_object_mc(C.byref(mc), buf, C.byref(size)) == 0
    a, b = tmp_path / "cd.co", tmp_path / "mc0.co"
    a.write_bytes(ref)
    b.write_bytes(buf.raw[:size.value])
    assert _meta(a) == _meta(b) and _bodies(a) == _bodies(b)
    c = tmp_path / "py0.co"
    c.write_bytes(E.code_object(JL.LQR, 2, 2, ranks=(4,), name="lqr_mc0", chain=False, **KW))
    assert _meta(a) == _meta(c) and _bodies(a) == _bodies(c)
    # ... and the same model id
    i0 = E.compile_model(JL.LQR, 2, 2, ranks=(4,), name="lqr_mc0", **KW)
    mid = C.c_int(0)
    assert L.c3sc_hip_model_compile_mc(C.byref(mc), C.byref(mid)) == 0 and mid.value == i0
    assert E.compile_model(JL.LQR, 2, 2, ranks=(4,), name="lqr_mc0", chain=True, **KW) != i0


@pytest.mark.parametrize("chain", [-1, 2, 7])
def test_bad_flag_values_are_argument_errors(chain):
    L = E.load_library()
    mc = _mc(chain, "lqr_mc_bad")
    mid, size = C.c_int(0), C.c_size_t(0)
    assert L.c3sc_hip_model_compile_mc(C.byref(mc), C.byref(mid)) == ERR_ARG
    assert L.c3sc_hip_model_code_object_mc(C.byref(mc), None, C.byref(size)) == ERR_ARG
    assert "chain must be 0 or 1" in L.c3sc_hip_model_log().decode()
    assert L.c3sc_hip_model_compile_mc(None, C.byref(mid)) == ERR_ARG
