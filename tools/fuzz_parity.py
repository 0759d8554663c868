"""Randomised parity of every Bellman fiber kernel variant against the CPU oracle, the long-running form of
tests/test_gpu_random_sweep.py: the same generator and the same checker (tests/random_cases.py), walking seeds from `seed` upwards
over every family (the eleven built-in workloads and the forms leg: lqr_cd_jump, lqr_ic, lqgame) instead of the committed seed lists.  Values to 1e-12 of the scale, absorbed flags exact, controls equal where
the oracle pins them, the kernel name and every refusal as the selection restatement predicts; nothing is skipped without a count.
    python tools/fuzz_parity.py [seconds] [seed]        walk seeds for `seconds` (120), from `seed` (1)
    python tools/fuzz_parity.py --case FAMILY SEED      replay one case, every launch printed
The summary counts launches and the worst relative error per kernel family, refusals by reason, and the draws the oracle does not
accept (a stationary candidate).  Exit status 1 on a failure; a device error that is no refusal ends the run at once (2)."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle_lib
import random_cases as R
from c3sc_amd.engine import C3scHipError


def summary(tally, ncase, nrejected, nfail, t0):
    for line in tally.lines():
        print(line)
    print(f"{ncase} random problems, {sum(tally.runs.values())} kernel runs, {sum(tally.refused.values())} refused as predicted, "
          f"{nrejected} draws the oracle does not accept, {nfail} failures, worst relative error {max(tally.worst.values(), default=0.0):.3e}, "
          f"{time.time() - t0:.0f} s")


def main(argv):
    oracle_lib.build()
    t0 = time.time()
    tally = R.Tally()
    make = lambda family, seed: R.case(family, seed) if family in R.FAMILIES else R.form_case(family, seed)
    run = lambda c, **kw: R.run_case(c, tally, **kw) if c.family in R.FAMILIES else R.run_form_case(c, tally, **kw)
    if argv[:1] == ["--case"]:
        c = make(argv[1], int(argv[2]))
        print(repr(c))
        try:
            run(c, verbose=True)
        except AssertionError as e:
            print("FAIL", e)
            return 1
        summary(tally, 1, 0, 0, t0)
        return 0
    budget = float(argv[0]) if argv else 120.0
    seed = int(argv[1]) if len(argv) > 1 else 1
    ncase = nfail = nrejected = 0
    last_note = t0
    while time.time() - t0 < budget:
        for family in R.FAMILIES + R.FORM_FAMILIES:
            c = make(family, seed)
            try:
                run(c)
                ncase += 1
            except R.Rejected:
                nrejected += 1
            except AssertionError as e:
                ncase += 1
                nfail += 1
                print("FAIL", e, flush=True)
            except C3scHipError as e:  # no refusal of launch_bellman's: nothing more is started on the device
                print("DEVICE ERROR", repr(c), e, flush=True)
                summary(tally, ncase, nrejected, nfail + 1, t0)
                return 2
            if time.time() - last_note > 30.0:  # a silent GPU job is taken to be hung
                print(f"... seed {seed}: {ncase} problems, {sum(tally.runs.values())} kernel runs, {nfail} failures, {time.time() - t0:.0f} s", flush=True)
                last_note = time.time()
            if time.time() - t0 >= budget:
                break
        seed += 1
    summary(tally, ncase, nrejected, nfail, t0)
    return 1 if nfail else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
