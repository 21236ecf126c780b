"""What the overlap (dovetail) mode of the long pairs costs.

Workload (seeded), alphabet 20, BLOSUM62, affine -11/-1 and linear -11/-11, everything device-resident:
  two 20 000-letter reads that share a 10 000-letter dovetail (Y's tail, mutated 15 % / 2 %, is X's head);
  two 50 000-letter sequences that share 25 000 letters the same way;
  a 20 000-letter read (rows) hanging 5 000 letters over the end of a 200 000-letter contig (columns).
Per pair and gap model:
  Engine.score_overlap_dev's kernel time beside Engine.score_semi_dev's and beside Engine.score_dev's
  global kernel in one direction (GSA_SCORE_BIDI=0), in the same process on the same R x C and rows
  per lane: the overlap instance is the semi-global one plus the selects of at most nine blocks per
  strip and one store per lane and strip;
  Engine.align_pair_overlap_dev: score, fill and walk times and the move codes held.

Method: one untimed pass, then --repeats timed passes; the hipEvent times the calls
report and the host clock around the synchronous calls; medians and the spread (max - min).  Every
CIGAR is replayed on the host (tests/_overlap_oracle.replay) and must give the call's score and cells.
Prints a table and one JSON line and writes the table to profiles/align_pair_overlap_ab.txt (--out)."""
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
# (label, R, C, shared letters, X's tail on Y's head instead of Y's tail on X's head)
PAIRS = [("20k x 20k, 10k shared", 20000, 20000, 10000, False), ("50k x 50k, 25k shared", 50000, 50000, 25000, False),
         ("20k over 200k's end", 20000, 200000, 15000, True)]


def make_pair(F, R, C, shared, tail_of_x, seed):
    core = F.synthetic_seq(shared, seed)
    mut = F.mutate_seq(core, seed + 1)[1:]
    if not tail_of_x:
        y = np.concatenate([F.synthetic_seq(R, seed + 2)[1:], core[1:]])[-R:]
        x = np.concatenate([mut, F.synthetic_seq(C, seed + 3)[1:]])[:C]
    else:
        y = np.concatenate([mut, F.synthetic_seq(R, seed + 2)[1:]])[:R]
        x = np.concatenate([F.synthetic_seq(C, seed + 3)[1:], core[1:]])[-C:]
    hdr = lambda a: np.concatenate([[0], a]).astype(np.int32)
    return hdr(y), hdr(x)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--pairs", type=int, nargs="*", default=[0, 1, 2], help="indices into the pair list")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_pair_overlap_ab.txt"), help="the table's file ('' for none)")
    a = ap.parse_args()
    assert a.repeats >= 3

    import torch
    import gpuseqalign_amd as gsa
    from gpuseqalign_amd import formats as F
    from tests import _overlap_oracle as oo

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
            label, R, C, shared, tail_of_x = PAIRS[idx]
            Y, X = make_pair(F, R, C, shared, tail_of_x, 3000 + 10 * idx)
            ty, tx = torch.from_numpy(Y).to(dev), torch.from_numpy(X).to(dev)
            torch.cuda.synchronize(dev)
            args = (ty.data_ptr(), len(Y), tx.data_ptr(), len(X), ts.data_ptr(), substsz)
            for name, go, ge in GAPS:
                def over():
                    r = eng.score_overlap_dev(*args, go, ge)
                    return r, {"kernel_ms": r["kernel_ms"]}

                def semi():
                    r = eng.score_semi_dev(*args, go, ge)
                    return r, {"kernel_ms": r["kernel_ms"]}

                def glob():
                    r = eng.score_dev(*args, go, ge, False)
                    return r, {"kernel_ms": r["kernel_ms"]}

                def align():
                    r = eng.align_pair_overlap_dev(*args, go, ge)
                    align.info = eng.last_align_pair_overlap_info()
                    return r, {k: align.info[k] for k in ("score_ms", "fill_ms", "walk_ms")}

                eng.set_knob("GSA_SCORE_BIDI", "0")  # the global score in one direction, as the other two run
                _, gms = timed(glob)
                launch = eng.last_launch()
                eng.set_knob("GSA_SCORE_BIDI", None)
                _, sms = timed(semi)
                ores, oms = timed(over)
                res, ams = timed(align)
                info = align.info
                got = (res["score"], res["i_start"], res["j_start"], res["i_end"], res["j_end"], res["cigar"])
                assert res["status"] == 0 and (res["score"], res["i_end"], res["j_end"]) == (ores["score"], ores["i_end"], ores["j_end"])
                assert (res["i_start"] == 0 or res["j_start"] == 0) and (res["i_end"] == R or res["j_end"] == C)
                assert oo.replay(Y, X, sub, go, ge, got) == res["score"]
                row = {"pair": label, "gaps": name, "rows": R, "cols": C, "k": launch.get("k", 0), "score": res["score"],
                       "start": [res["i_start"], res["j_start"]], "end": [res["i_end"], res["j_end"]],
                       "strip_rows": info["strip_rows"], "strips": info["strips"], "strips_filled": info["strips_filled"],
                       "chunks": info["chunks"], "code_mib": round(info["code_bytes"] / 2 ** 20, 1),
                       "overlap_over_semi": round(oms["kernel_ms"][0] / sms["kernel_ms"][0], 3),
                       "overlap_over_global": round(oms["kernel_ms"][0] / gms["kernel_ms"][0], 3),
                       "fill_gcups": round(res["i_end"] * res["j_end"] / ams["fill_ms"][0] / 1e6, 1)}
                for tag, ms in (("overlap", oms), ("semi", sms), ("global", gms), ("align", ams)):
                    for k, v in ms.items():
                        row[tag + "_" + k], row[tag + "_" + k + "_spread"] = round(v[0], 3), round(v[1], 3)
                rows.append(row)
            del ty, tx

    lines = []
    lines.append("the shared letters are a mutated copy (15 %% substitutions, 2 %% indels), BLOSUM62, device-resident; "
                 "one untimed pass, then %d timed: medians (spread = max - min)" % a.repeats)
    lines.append("overlap = Engine.score_overlap_dev's kernels (fill + maximum over row R and column C); semi = Engine.score_semi_dev's; "
                 "global = Engine.score_dev, global, one direction (GSA_SCORE_BIDI=0); the same R x C and rows per lane K, one process; "
                 "align = Engine.align_pair_overlap_dev; every CIGAR replayed on the host")
    lines.append("pair                   gaps    K   start cell      end cell | overlap kernel ms (spread)  semi kernel ms (spread) "
                 "global kernel ms (spread) overlap/semi overlap/global | align call ms  score ms   fill ms (spread)   "
                 "walk ms (spread) fill GCUPS | TR strips filled chunks codes MiB")
    for r in rows:
        lines.append(f"{r['pair']:22s} {r['gaps']:6s} {r['k']:2d} {str(tuple(r['start'])):>14s} {str(tuple(r['end'])):>16s} | "
                     f"{r['overlap_kernel_ms']:17.3f} ({r['overlap_kernel_ms_spread']:6.3f}) {r['semi_kernel_ms']:15.3f} "
                     f"({r['semi_kernel_ms_spread']:6.3f}) {r['global_kernel_ms']:16.3f} ({r['global_kernel_ms_spread']:6.3f}) "
                     f"{r['overlap_over_semi']:12.3f} {r['overlap_over_global']:14.3f} | {r['align_call_ms']:13.3f} "
                     f"{r['align_score_ms']:9.3f} {r['align_fill_ms']:9.3f} ({r['align_fill_ms_spread']:6.3f}) "
                     f"{r['align_walk_ms']:9.3f} ({r['align_walk_ms_spread']:6.3f}) {r['fill_gcups']:10.1f} | "
                     f"{r['strip_rows']:4d} {r['strips']:6d} {r['strips_filled']:6d} {r['chunks']:6d} {r['code_mib']:9.1f}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps({"tool": "align_pair_overlap_bench", "repeats": a.repeats, "rows": rows}), flush=True)


if __name__ == "__main__":
    main()
