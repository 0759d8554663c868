"""The form mask of the Bellman backup and its rule (kernel_common.hpp: FORM_*, model_form, form_offered), checked
by the compiler on a translation unit of static_asserts: no GPU is needed.  form_offered accepts exactly the 19 masks listed here
and rejects the other 45, k_rollout has 11 of them, k_rollout_ode 2 and the control-box minimiser the plain form only; model_form
reads the wrappers' bits; KArgs keeps its size.  The lists are written out, not computed from the rule."""
import json
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G, H, S, J, I, C = 1, 2, 4, 8, 16, 32  # FORM_GAME, FORM_HORIZON, FORM_STOP, FORM_JUMP, FORM_IMPULSE, FORM_CORR
# the per-wave kernels: the plain form, the game alone, impulse control alone or with jumps, every subset of {horizon, stop, jump, corr}
PER_WAVE = [0, G, I, I | J,
            H, S, H | S, J, H | J, S | J, H | S | J,
            C, C | H, C | S, C | H | S, C | J, C | H | J, C | S | J, C | H | S | J]
ROLLOUT = [0, G, I, I | J, H, S, H | S, J, H | J, S | J, H | S | J]  # those without corr
ROLLOUT_ODE = [0, G]
BOX = [0]


def _asserts(kind, offered):
    assert len(set(offered)) == len(offered)
    return "".join(f"static_assert({'' if m in offered else '!'}c3sc::form_offered({m}u, c3sc::{kind}), \"{kind} {m}\");\n" for m in range(64))


def test_the_rule_offers_exactly_the_listed_forms(tmp_path):
    assert (len(PER_WAVE), len(ROLLOUT), len(ROLLOUT_ODE), len(BOX)) == (19, 11, 2, 1)
    bits = "".join(f"static_assert(c3sc::FORM_{n} == {v}u);\n"
                   for n, v in (("GAME", G), ("HORIZON", H), ("STOP", S), ("JUMP", J), ("IMPULSE", I), ("CORR", C), ("ALL", 63)))
    src = tmp_path / "form_rule.hip"
    src.write_text('#include "kernel_common.hpp"\n' + bits
                   + "".join(f"static_assert({'' if m in PER_WAVE else '!'}c3sc::form_offered({m}u), \"default kind {m}\");\n" for m in range(64))
                   + _asserts("FORM_PER_WAVE", PER_WAVE) + _asserts("FORM_ROLLOUT", ROLLOUT)
                   + _asserts("FORM_ROLLOUT_ODE", ROLLOUT_ODE) + _asserts("FORM_BOX", BOX)
                   + "static_assert(!c3sc::form_offered(64u) && !c3sc::form_offered(128u | c3sc::FORM_STOP) && !c3sc::form_offered(~0u));\n"
                   "using namespace c3sc;\nstruct M0 {};\n"
                   "static_assert(model_form<M0>() == 0u);\n"
                   "static_assert(model_form<GameOf<M0>>() == FORM_GAME);\n"
                   "static_assert(model_form<ImpulseOf<JumpOf<M0>>>() == (FORM_IMPULSE | FORM_JUMP));\n"
                   "static_assert(model_form<CorrOf<JumpOf<StopOf<HorizonOf<M0>>>>>() == (FORM_HORIZON | FORM_STOP | FORM_JUMP | FORM_CORR));\n"
                   "static_assert(form_offered(model_form<CorrOf<JumpOf<StopOf<HorizonOf<M0>>>>>()));\n"
                   "static_assert(model_corr<CorrOf<JumpOf<M0>>>() && model_jump<CorrOf<JumpOf<M0>>>() && !model_stop<CorrOf<JumpOf<M0>>>());\n"
                   "static_assert(sizeof(KArgs) == 1368);\n")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    r = subprocess.run([hipcc, "-std=c++20", "-x", "hip", "--offload-arch=gfx950", "-fsyntax-only",
                        "-I", os.path.join(ROOT, "c3sc_amd", "csrc"), "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


@pytest.mark.parametrize("spec", ["form_hsjc", "form_ij"])
def test_code_object_holds_exactly_the_kernels_of_the_manifest(tmp_path, spec):
    """the mangled names of a model's kernels at rank 4, for the fullest spec without impulse control (horizon, stop, jumps and
    a correlated pair) and for impulse control with jumps, against tests/golden/rtc_form_manifest.json: a form dropped or added
    in any combination of features changes the set.  The rollouts' names carry the model id, which counts the models this
    process compiled before: it is written <id> on both sides."""
    from c3sc_amd import engine as E
    import corr_lib as CL
    import impulse_lib as IL
    import jump_lib as JL
    from test_rtc_model_build import _meta

    if spec == "form_hsjc":
        co = E.code_object(CL.LQR_JUMP, 2, 2, ranks=(4,), name=spec, horizon=True, stop=True, njump=JL.LQR_NJUMP, corr_pairs=CL.LQR_PAIRS,
                           **CL.LQR_MASKS)
    else:
        co = E.code_object(IL.LQR_JUMP, 2, 2, ranks=(4,), name=spec, njump=JL.LQR_NJUMP, nimpulse=IL.LQR_NIMPULSE, **IL.LQR_MASKS)
    p = tmp_path / (spec + ".co")
    p.write_bytes(co)
    names = sorted(re.sub(r"(k_rollout(?:_ode)?)ILi\d+E", r"\1ILi<id>E", k) for k in _meta(p) if "RtcModel" in k)
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "rtc_form_manifest.json")))[spec]
    assert len(want) == {"form_hsjc": 41, "form_ij": 13}[spec]
    assert names == want, (sorted(set(names) - set(want)), sorted(set(want) - set(names)))
