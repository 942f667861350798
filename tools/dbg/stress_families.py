"""Long runs of the seeded family sweeps (tests/sweep_cases.py): N drawn rows of every sweep, or of the sweeps named, through the
runners of tests/family_runners.py against the references and bars of the families' tables - what tests/test_gpu_family_sweeps.py
does with 24 rows of seeds 1 and 2.  Prints one line per mismatch (sweep, seed, index and the row: sweep_cases.draw rebuilds it),
then `failures: K`; exits non-zero on a mismatch and stops at the first call that returns a HIP error.  Not run by the suite.
python tools/dbg/stress_families.py SEED N [sweep ...]"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "hyperspectral_super-resolution_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import torch
import sweep_cases as sw
from family_runners import JUDGES, LAUNCH_READERS
from gpu_harness import LaunchLog, lib

seed, n = int(sys.argv[1]), int(sys.argv[2])
sweeps = sys.argv[3:] or list(sw.SWEEPS)
assert set(sweeps) <= set(sw.SWEEPS), sorted(sw.SWEEPS)
bad = 0


class StopLog(LaunchLog):
    """The checked call, ending the run at the first entry point that returns HSR_ERR_HIP (3)."""

    def call(self, expect, fn, *args):
        def checked(*a):
            rc = fn(*a)
            if rc == 3:
                print("HIP ERROR", lib().hsr_last_error(), "after %d failures: stopping; failures: %d" % (bad, bad + 1), flush=True)
                sys.exit(2)
            return rc
        super().call(expect, checked, *args)


logs = {family: StopLog(reader, joined=joined) for family, (reader, joined) in LAUNCH_READERS.items()}
for sweep in sweeps:
    S = sw.SWEEPS[sweep]
    skipped, worst = 0, 0.0
    for index in range(n):
        row = sw.draw(sweep, seed, index)
        case = sw.case(sweep, row)
        if not S.admitted(row, case):
            skipped += 1
            continue
        try:
            worst = max(worst, JUDGES[sweep](torch, row, case, logs[S.family]))
            torch.cuda.synchronize()
        except AssertionError as e:
            bad += 1
            print("MISMATCH", sweep, seed, index, str(e)[:400], "row:", row, flush=True)
        except RuntimeError as e:                                    # torch reports a HIP error of an earlier launch
            print("HIP ERROR", sweep, seed, index, str(e)[:400], "row:", row, "failures:", bad + 1, flush=True)
            sys.exit(2)
    print(f"{sweep}: {n - skipped} rows run, {skipped} skipped, worst |err| / bar {worst:.3g}", flush=True)
print("family stress done; failures:", bad, flush=True)
sys.exit(1 if bad else 0)
