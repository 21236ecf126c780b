"""What the semi-global mode of the long pairs costs.

Workload (seeded), alphabet 20, BLOSUM62, affine -11/-1 and linear -11/-11, everything device-resident:
  a 20 000-letter query, a mutated copy (15 % substitutions, 2 % indels) of a stretch of the subject,
  in subjects of 200 000 and 1 000 000 letters (the stretch begins at 3/4 of the subject);
  a related pair of 50 000 x 50 000 letters.
Per pair and gap model:
  Engine.score_semi_dev's kernel time beside Engine.score_dev's global kernel in one direction
  (GSA_SCORE_BIDI=0) for the same R x C on the same device: the same K-rows kernel without the row
  capture and the row maximum, the only fair yardstick of the new instances;
  Engine.align_pair_semi_dev: score, fill and walk times, the move codes held with the window and what
  they would be without it (j_end TR / 2 per strip: arithmetic only).

Method: one untimed pass, then --repeats timed passes; the hipEvent times the calls
report and the host clock around the synchronous calls; medians and the spread (max - min).  Every
CIGAR is replayed on the host (tests/_align_oracle.rescore) and must give the call's score and end cell.
Prints a table and one JSON line and writes the table to profiles/align_pair_semi_ab.txt (--out)."""
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

GAPS = [("affine", -11, -1), ("linear", -11, -11)]
PAIRS = [("20k in 200k", 20000, 200000), ("20k in 1M", 20000, 1000000), ("50k x 50k", 50000, 50000)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--pairs", type=int, nargs="*", default=[0, 1, 2], help="indices into the pair list")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_pair_semi_ab.txt"), help="the table's file ('' for none)")
    a = ap.parse_args()

    import torch
    import gpuseqalign_amd as gsa
    from gpuseqalign_amd import formats as F
    from tests import _align_oracle as ao

    assert torch.cuda.is_available(), "needs cuda:0"
    dev = torch.device("cuda:0")
    sub = F.read_subst_json(os.path.join(ROOT, "tests", "golden", "resrc", "subst.json")).matrix("blosum62")
    substsz = int(round(sub.size ** 0.5))
    ts = torch.from_numpy(np.ascontiguousarray(sub, dtype=np.int32).ravel().copy()).to(dev)

    def timed(fn):
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
        for idx in a.pairs:
            label, R, C = PAIRS[idx]
            X = F.synthetic_seq(C, 1000 + idx)
            at = 0 if R == C else (3 * C) // 4
            Y = F.mutate_seq(np.concatenate([[0], X[1 + at:1 + at + R]]).astype(np.int32), 2000 + idx)
            ty, tx = torch.from_numpy(Y).to(dev), torch.from_numpy(X).to(dev)
            torch.cuda.synchronize(dev)
            args = (ty.data_ptr(), len(Y), tx.data_ptr(), len(X), ts.data_ptr(), substsz)
            for name, go, ge in GAPS:
                def semi():
                    r = eng.score_semi_dev(*args, go, ge)
                    return r, {"kernel_ms": r["kernel_ms"]}

                def glob():
                    r = eng.score_dev(*args, go, ge, False)
                    return r, {"kernel_ms": r["kernel_ms"]}

                def align():
                    r = eng.align_pair_semi_dev(*args, go, ge)
                    align.info = eng.last_align_pair_semi_info()
                    return r, {k: align.info[k] for k in ("score_ms", "fill_ms", "walk_ms")}

                eng.set_knob("GSA_SCORE_BIDI", "0")  # the global score in one direction, as the semi-global one runs
                gres, gms = timed(glob)
                launch = eng.last_launch()
                eng.set_knob("GSA_SCORE_BIDI", None)
                sres, sms = timed(semi)
                res, ams = timed(align)
                info = align.info
                assert res["status"] == 0 and (res["score"], res["i_end"], res["j_end"]) == (sres["score"], sres["i_end"], sres["j_end"])
                assert res["i_start"] == 0 and res["i_end"] == len(Y) - 1
                assert ao.rescore(res["cigar"], Y, X, 0, res["j_start"], sub, go, ge) == (res["score"], res["i_end"], res["j_end"])
                tr = info["strip_rows"]
                row = {"pair": label, "gaps": name, "rows": len(Y) - 1, "cols": len(X) - 1, "k": launch.get("k", 0),
                       "score": res["score"], "j_start": res["j_start"], "j_end": res["j_end"], "j_window": info["j_window"],
                       "strip_rows": tr, "strips": info["strips"], "chunks": info["chunks"],
                       "code_mib": round(info["code_bytes"] / 2 ** 20, 1),
                       "code_mib_no_window": round(res["j_end"] * (tr // 2) * info["strips"] / 2 ** 20, 1),
                       "semi_over_global": round(sms["kernel_ms"][0] / gms["kernel_ms"][0], 3),
                       "fill_gcups": round((len(Y) - 1) * (res["j_end"] - info["j_window"]) / ams["fill_ms"][0] / 1e6, 1)}
                for k, v in sms.items():
                    row["semi_" + k], row["semi_" + k + "_spread"] = round(v[0], 3), round(v[1], 3)
                for k, v in gms.items():
                    row["global_" + k], row["global_" + k + "_spread"] = round(v[0], 3), round(v[1], 3)
                for k, v in ams.items():
                    row["align_" + k], row["align_" + k + "_spread"] = round(v[0], 3), round(v[1], 3)
                rows.append(row)
            del ty, tx

    lines = []
    lines.append("query = a mutated copy (15 %% substitutions, 2 %% indels) of a stretch of the subject, BLOSUM62, device-resident; "
                 "one untimed pass, then %d timed: medians (spread = max - min)" % a.repeats)
    lines.append("semi = Engine.score_semi_dev's kernels (fill + row maximum); global = Engine.score_dev, global, one direction "
                 "(GSA_SCORE_BIDI=0), the same R x C and rows per lane; align = Engine.align_pair_semi_dev; every CIGAR replayed on the host")
    lines.append("pair        gaps    K     j_end  j_window | semi kernel ms (spread) global kernel ms (spread) semi/global | "
                 "align call ms  score ms   fill ms (spread)   walk ms (spread) fill GCUPS | TR strips chunks codes MiB  without window MiB")
    for r in rows:
        lines.append(f"{r['pair']:11s} {r['gaps']:6s} {r['k']:2d} {r['j_end']:9d} {r['j_window']:9d} | "
                     f"{r['semi_kernel_ms']:14.3f} ({r['semi_kernel_ms_spread']:6.3f}) {r['global_kernel_ms']:16.3f} "
                     f"({r['global_kernel_ms_spread']:6.3f}) {r['semi_over_global']:11.3f} | {r['align_call_ms']:13.3f} "
                     f"{r['align_score_ms']:9.3f} {r['align_fill_ms']:9.3f} ({r['align_fill_ms_spread']:6.3f}) "
                     f"{r['align_walk_ms']:9.3f} ({r['align_walk_ms_spread']:6.3f}) {r['fill_gcups']:10.1f} | "
                     f"{r['strip_rows']:4d} {r['strips']:6d} {r['chunks']:6d} {r['code_mib']:9.1f} {r['code_mib_no_window']:19.1f}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps({"tool": "align_pair_semi_bench", "repeats": a.repeats, "rows": rows}), flush=True)


if __name__ == "__main__":
    main()
