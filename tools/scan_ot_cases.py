#!/usr/bin/env python3
"""Finds the late-breakdown and convergence rows of tests/ot_cases.py (CPU only, long double; about a minute).

  python tools/scan_ot_cases.py

Breakdown rows: for n x m in {130 x 66, 97 x 65}, reg in {0.01, 0.05}, the moved point in X or in Y and seed 0..199 (t = 700 + seed)
it runs ot_cases.solve and keeps an input only if
  * it breaks down at an iteration > 0,
  * |ln(q / DBL_MAX)| >= 100 MARGIN at every iteration up to the break (q: the largest element of the updated v and u), and
  * the break iteration stays where it is when every element of K moves by +4, by -4 and by a random +-4 spacings.
Per class (odd through v, even, multiple of 10, through u alone, odd past iteration 11) it prints the candidate with the widest
margin as a line for ROWS.  Convergence rows: the error of every check of two shapes, and a threshold between two of them."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import ot_cases as oc  # noqa: E402


def stable(X, Y, reg, ref):
    for how in (1, -1, 0):
        got = oc.solve(X, Y, reg, 40, 1e-9, K=oc.perturbed(ref["K"], how), upto=ref["break_iter"] + 2)
        if got["break_iter"] != ref["break_iter"]:
            return False
    return True


def main():
    found = []
    for (n, m) in ((130, 66), (97, 65)):
        for reg in (0.01, 0.05):
            for side in "XY":
                for seed in range(200):
                    t = 700.0 + seed
                    X, Y = oc.breakdown_clouds(n, m, seed, side, t, reg)
                    ref = oc.solve(X, Y, reg, 40, 1e-9)
                    bi = ref["break_iter"]
                    if not bi:
                        continue
                    margin = min(abs(q) for q in ref["q"])
                    if margin < 100 * oc.MARGIN or not stable(X, Y, reg, ref):
                        continue
                    found.append((margin, n, m, seed, side, t, reg, bi, ref["through"]))
    print("stable breakdown inputs: %d; break iterations %s" % (len(found), sorted({f[7] for f in found})))
    print("through u alone at", sorted({f[7] for f in found if f[8] == "u"}), "; multiples of 10:", sorted({f[7] for f in found if f[7] % 10 == 0}))
    classes = {"odd-v": lambda b, th: b % 2 == 1 and th == "v" and b <= 9, "even": lambda b, th: b % 2 == 0 and b % 10 != 0,
               "tenth": lambda b, th: b % 10 == 0, "u-odd": lambda b, th: th == "u" and b % 2 == 1 and b <= 9,
               "u-even": lambda b, th: th == "u" and b % 2 == 0 and b <= 9, "late": lambda b, th: b > 11 and b % 2 == 1}
    for cname, pred in classes.items():
        best = max((f for f in found if pred(f[7], f[8])), default=None)
        if best is None:
            print("# %s: none in 200 seeds" % cname)
            continue
        margin, n, m, seed, side, t, reg, bi, th = best
        print('    "break%d-%s": _brk(%d, %d, %d, "%s", %.1f, %g, %d, "%s"),      # %s; margin %.3g' % (bi, th, n, m, seed, side, t, reg, bi, th, cname, margin))
    for (n, m) in ((61, 66), (70, 646)):
        X, Y = oc.clouds(n, m, n + m)
        ref = oc.solve(X, Y, 0.05, 35, 0.0)
        print("# %dx%d: (iteration, err, bound)" % (n, m), ["(%d, %.4g, %.2g)" % e for e in ref["errs"]])
        for (i0, e0, _), (i1, e1, b1) in zip(ref["errs"], ref["errs"][1:]):
            print("#   stopThr %.2g converges at %d" % (float("%.2g" % np.sqrt(e0 * e1)), i1))


if __name__ == "__main__":
    main()
