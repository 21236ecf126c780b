"""What the banded calls cost beside the unbanded ones on related long pairs.

Workload (seeded): a related pair of n x n letters (seqY a mutated copy of seqX: 15 % substitutions, 2 %
indels, as tools/align_pair_bench.py makes them), n = 50 000, 200 000 and 1 000 000; BLOSUM62 over 20
letters with gaps -11 / -1, and a DNA table (match 2, mismatch -3) over 4 letters with gaps -5 / -2;
band = 512 and band = 2048 diagonals on either side of the ones (0, 0) and (R, C) need.  Everything
device-resident, one process.

Per pair and band: Engine.score_band_dev and Engine.align_pair_band_dev (fill with codes + walk).  The
yardsticks run in the same process on the same pair and come from the unbanded calls alone:
Engine.score_dev (default settings) and, up to --align-max letters, Engine.align_pair_dev with its score +
fill + walk split.  Derived: the fill's time per super-step and per in-band cell, the walk's time per move,
the bytes of codes.

Method: one untimed pass, then --repeats timed passes; the hipEvent times the calls
report and the host clock around the synchronous calls; medians and the spread (max - min).  Every banded
CIGAR is replayed on the host and must give the call's score.  Prints a table and one JSON line and
writes the table to profiles/align_pair_band_ab.txt (--out)."""
import argparse
import gc
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[50000, 200000, 1000000])
    ap.add_argument("--bands", type=int, nargs="*", default=[512, 2048])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--align-max", type=int, default=200000, help="largest n on which Engine.align_pair_dev is run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_pair_band_ab.txt"), help="the table's file ('' for none)")
    a = ap.parse_args()

    import torch
    import gpuseqalign_amd as gsa
    from gpuseqalign_amd import formats as F
    from tests import _align_oracle as ao

    assert torch.cuda.is_available(), "needs cuda:0"
    dev = torch.device("cuda:0")
    blosum = F.read_subst_json(os.path.join(ROOT, "tests", "golden", "resrc", "subst.json")).matrix("blosum62")
    blosum = np.ascontiguousarray(blosum, dtype=np.int32).reshape(int(round(blosum.size ** 0.5)), -1)
    dna = np.full((4, 4), -3, np.int32)
    np.fill_diagonal(dna, 2)
    tables = [("BLOSUM62", blosum, 20, -11, -1), ("DNA", dna, 4, -5, -2)]

    def timed(fn):
        """fn -> (value, {name: (median ms, spread ms)}); one untimed pass, then the timed ones."""
        acc, val = {}, None
        for it in range(1 + a.repeats):
            gc.collect()
            gc.disable()
            try:
                t0 = time.perf_counter()
                val, ms = fn()
                ms["call_ms"] = (time.perf_counter() - t0) * 1e3
            finally:
                gc.enable()
            if it:
                for k, v in ms.items():
                    acc.setdefault(k, []).append(v)
        return val, {k: (statistics.median(v), max(v) - min(v)) for k, v in acc.items()}

    rows = []
    with gsa.Engine(0) as eng:
        for tname, sub, alphabet, go, ge in tables:
            ts = torch.from_numpy(sub.ravel().copy()).to(dev)
            for n in a.sizes:
                X = F.synthetic_seq(n, 1000 + n, alphabet)
                Y = F.mutate_seq(X, 2000 + n, alphabet=alphabet)
                R, C = len(Y) - 1, len(X) - 1
                ty, tx = torch.from_numpy(Y).to(dev), torch.from_numpy(X).to(dev)
                torch.cuda.synchronize(dev)
                args = (ty.data_ptr(), len(Y), tx.data_ptr(), len(X), ts.data_ptr(), len(sub))

                def score():
                    r = eng.score_dev(*args, go, ge)
                    return r, {"kernel_ms": r["kernel_ms"]}

                sres, sms = timed(score)
                ares = ams = None
                if n <= a.align_max:
                    def align():
                        r = eng.align_pair_dev(*args, go, ge)
                        info = eng.last_align_pair_info()
                        return r, {k: info[k] for k in ("score_ms", "fill_ms", "walk_ms")}

                    ares, ams = timed(align)
                    assert ares["status"] == 0 and ares["score"] == sres["score"]
                for band in a.bands:
                    lo, hi = min(0, C - R) - band, max(0, C - R) + band

                    def bscore():
                        r = eng.score_band_dev(*args, go, ge, lo, hi)
                        return r, {"kernel_ms": r["kernel_ms"]}

                    def balign():
                        r = eng.align_pair_band_dev(*args, go, ge, lo, hi, 8 << 30)
                        info = eng.last_align_pair_band_info()
                        balign.info = info
                        return r, {k: info[k] for k in ("score_ms", "walk_ms")}

                    bs, bsms = timed(bscore)
                    ba, bams = timed(balign)
                    info = balign.info
                    assert ba["status"] == 0 and ba["score"] == bs["score"] <= sres["score"]
                    assert ao.rescore(ba["cigar"], Y, X, 0, 0, sub, go, ge) == (ba["score"], R, C)
                    moves = sum(c for c, _ in ao.runs(ba["cigar"]))
                    W = info["band_hi"] - info["band_lo"] + 1
                    row = {"table": tname, "n": n, "rows": R, "cols": C, "band": band, "diagonals": W,
                           "strips": info["strips"], "waves": info["waves"], "supersteps": info["supersteps"],
                           "code_mib": round(info["code_bytes"] / 2 ** 20, 1), "proved_optimal": info["proved_optimal"],
                           "same_score_as_unbanded": int(ba["score"] == sres["score"]),
                           "same_cigar_as_unbanded": (int(ba["cigar"] == ares["cigar"]) if ares else -1), "moves": moves,
                           "band_score_ms": round(bsms["kernel_ms"][0], 3), "band_score_ms_spread": round(bsms["kernel_ms"][1], 3),
                           "band_score_call_ms": round(bsms["call_ms"][0], 3),
                           "band_fill_ms": round(bams["score_ms"][0], 3), "band_fill_ms_spread": round(bams["score_ms"][1], 3),
                           "band_walk_ms": round(bams["walk_ms"][0], 3), "band_walk_ms_spread": round(bams["walk_ms"][1], 3),
                           "band_align_call_ms": round(bams["call_ms"][0], 3), "band_align_call_ms_spread": round(bams["call_ms"][1], 3),
                           "score_us_per_superstep": round(1e3 * bsms["kernel_ms"][0] / info["supersteps"], 2),
                           "fill_us_per_superstep": round(1e3 * bams["score_ms"][0] / info["supersteps"], 2),
                           "fill_ns_per_cell": round(1e6 * bams["score_ms"][0] / (R * W), 3),
                           "walk_us_per_move": round(1e3 * bams["walk_ms"][0] / moves, 3),
                           "score_dev_kernel_ms": round(sms["kernel_ms"][0], 3), "score_dev_kernel_ms_spread": round(sms["kernel_ms"][1], 3),
                           "score_dev_call_ms": round(sms["call_ms"][0], 3)}
                    if ams:
                        for k, v in ams.items():
                            row["align_pair_" + k] = round(v[0], 3)
                        row["align_pair_call_ms_spread"] = round(ams["call_ms"][1], 3)
                    rows.append(row)
                del ty, tx

    lines = []
    lines.append("related pairs n x n (15 %% substitutions, 2 %% indels), device-resident, one process; one untimed pass, "
                 "then %d timed: medians (spread = max - min)" % a.repeats)
    lines.append("band = Engine.score_band_dev / Engine.align_pair_band_dev (fill with codes + walk), one workgroup; "
                 "yardsticks on the same pair in the same run: Engine.score_dev (kernel ms) and Engine.align_pair_dev "
                 "(call ms and its score + fill + walk); call ms: host clock around the synchronous call, the others hipEvent "
                 "times; every banded CIGAR replayed on the host")
    lines.append("table          n  band  diag strips supersteps codes MiB proved =score =cigar | band score call ms  kernel ms (spread) us/sstep | "
                 "band align call ms (spread) = fill ms (spread) us/sstep ns/cell + walk ms (spread) us/move | "
                 "score_dev call ms  kernel ms (spread) | align_pair_dev call ms (spread) = score + fill + walk")
    for r in rows:
        ap_ = ("%10.3f (%6.3f) = %9.3f + %9.3f + %9.3f" % (r["align_pair_call_ms"], r["align_pair_call_ms_spread"],
                                                             r["align_pair_score_ms"], r["align_pair_fill_ms"],
                                                             r["align_pair_walk_ms"])) if "align_pair_call_ms" in r else "not run"
        lines.append(f"{r['table']:8s} {r['n']:7d} {r['band']:5d} {r['diagonals']:5d} {r['strips']:6d} {r['supersteps']:10d} "
                     f"{r['code_mib']:9.1f} {r['proved_optimal']:6d} {r['same_score_as_unbanded']:6d} {r['same_cigar_as_unbanded']:6d} | "
                     f"{r['band_score_call_ms']:10.3f} {r['band_score_ms']:10.3f} ({r['band_score_ms_spread']:6.3f}) {r['score_us_per_superstep']:8.2f} | "
                     f"{r['band_align_call_ms']:10.3f} ({r['band_align_call_ms_spread']:6.3f}) = "
                     f"{r['band_fill_ms']:9.3f} ({r['band_fill_ms_spread']:6.3f}) {r['fill_us_per_superstep']:8.2f} "
                     f"{r['fill_ns_per_cell']:7.3f} + {r['band_walk_ms']:9.3f} ({r['band_walk_ms_spread']:6.3f}) "
                     f"{r['walk_us_per_move']:7.3f} | {r['score_dev_call_ms']:10.3f} {r['score_dev_kernel_ms']:10.3f} ({r['score_dev_kernel_ms_spread']:6.3f}) | {ap_}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps({"tool": "align_pair_band_bench", "sizes": a.sizes, "bands": a.bands, "repeats": a.repeats, "rows": rows}),
          flush=True)


if __name__ == "__main__":
    main()
