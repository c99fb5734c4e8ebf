"""CatchSyncSelectUsers detection counts on synthetic data: for each heuristic attacker (random,
average, bandwagon, segment; 50 profiles of 36 fillers, tests/_catchsync_probe.py) appended to synth.make("ml1m"), how many
fakes are among the 50 largest scores for the three scores at grid_bits 0..2 and min_items 20 / 30, beside DegSim low / high
(float64, k = 25).  Host only (numpy): the restatement of the definition, not the kernels.  One JSON line per setting.

    python scripts/cs_detection_probe.py [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    from tests import _catchsync_probe as Q

    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also append every JSON line to this file")
    a = ap.parse_args()
    out = open(a.out, "a") if a.out else None
    base = Q.clean()
    for kind in Q.ATTACKERS:
        for keep in ("all", "above4"):
            ptr, idx, U, I = Q.poisoned(kind, keep, base)
            lengths = sorted(set((ptr[U + 1:] - ptr[U:-1]).tolist()))
            low, high = Q.degsim_hits(ptr, idx, U, I)
            recs = [{"attacker": kind, "edges": keep, "profile_items": [lengths[0], lengths[-1]], "detector": "degsim", "low": low,
                     "high": high}]
            for bits in (0, 1, 2):
                for min_items in (20, 30):
                    recs.append(dict({"attacker": kind, "edges": keep, "detector": "catchsync", "grid_bits": bits,
                                      "min_items": min_items}, **Q.catchsync_hits(ptr, idx, U, I, bits, min_items)))
            for rec in recs:
                line = json.dumps(rec)
                print(line, flush=True)
                if out:
                    out.write(line + "\n")
    if out:
        out.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
