"""What the alignment of a long pair costs over its score.

Workload (seeded): a related pair of n x n letters (seqY a mutated copy of seqX: 15 % substitutions, 2 %
indels), alphabet 20, BLOSUM62; NW-LG and SW-LG -11/-11, NW-AG and SW-AG -11/-1; n = 10 000, 50 000 and
65 536 (whose codes are the default scratch limit, 2 GiB: a seqY that the indels made longer takes a
second chunk).  Everything device-resident.  Per
mode and size: Engine.align_pair_dev (score in one direction, fill, walk) beside Engine.score_dev on the
same pair (the split from both ends on, as users get it).  For NW-LG also the sparse fill plus the
device Trace2 (Engine.fill_sparse_dev, Engine.trace_sparse_dev) on the same pair.

Method: one untimed pass, then --repeats timed passes; host clock around the
synchronous calls and the hipEvent times the calls report; medians and the spread (max - min).  Every
CIGAR is replayed on the host (tests/_align_oracle.rescore) and must give the call's score and end cell.
Prints a table and one JSON line and writes the table to profiles/align_pair_ab.txt (--out)."""
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

MODES = [("NW-LG", -11, -11, False), ("NW-AG", -11, -1, False), ("SW-LG", -11, -11, True), ("SW-AG", -11, -1, True)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[10000, 50000, 65536])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--tile", type=int, default=256, help="tileBx of the sparse fill (NW-LG comparison)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_pair_ab.txt"), help="the table's file ('' for none)")
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
        for n in a.sizes:
            X = F.synthetic_seq(n, 1000 + n)
            Y = F.mutate_seq(X, 2000 + n)
            ty, tx = torch.from_numpy(Y).to(dev), torch.from_numpy(X).to(dev)
            torch.cuda.synchronize(dev)
            args = (ty.data_ptr(), len(Y), tx.data_ptr(), len(X), ts.data_ptr(), substsz)
            for name, go, ge, local in MODES:
                def score():
                    r = eng.score_dev(*args, go, ge, local)
                    return r, {"kernel_ms": r["kernel_ms"]}

                def align():
                    r = eng.align_pair_dev(*args, go, ge, local)
                    info = eng.last_align_pair_info()
                    align.info = info
                    return r, {k: info[k] for k in ("score_ms", "fill_ms", "walk_ms")}

                sres, sms = timed(score)
                both_ends = eng.last_launch().get("both_ends", 0)
                res, ams = timed(align)
                info = align.info
                assert res["status"] == 0 and info["chunks"] >= 1, (res["status"], info)
                assert (res["score"], res["i_end"], res["j_end"]) == (sres["score"], sres["i_end"], sres["j_end"])
                assert ao.rescore(res["cigar"], Y, X, res["i_start"], res["j_start"], sub, go, ge) == \
                    (res["score"], res["i_end"], res["j_end"])
                cells = res["i_end"] * res["j_end"]
                row = {"mode": name, "n": n, "rows": len(Y) - 1, "cols": len(X) - 1, "strip_rows": info["strip_rows"],
                       "strips": info["strips"], "chunks": info["chunks"], "code_mib": round(info["code_bytes"] / 2 ** 20, 1),
                       "moves": sum(c for c, _ in ao.runs(res["cigar"])), "score_dev_both_ends": int(both_ends),
                       "fill_gcups": round(cells / ams["fill_ms"][0] / 1e6, 1)}
                for k, v in ams.items():
                    row["align_" + k], row["align_" + k + "_spread"] = round(v[0], 3), round(v[1], 3)
                for k, v in sms.items():
                    row["score_" + k], row["score_" + k + "_spread"] = round(v[0], 3), round(v[1], 3)
                row["align_over_score"] = round(ams["call_ms"][0] / sms["call_ms"][0], 2)
                if name == "NW-LG":
                    geom = gsa.sparse_geometry(len(Y), len(X), a.tile)
                    hr = torch.empty(geom.hrowElems, dtype=torch.int32, device=dev)
                    hc = torch.empty(geom.hcolElems, dtype=torch.int32, device=dev)

                    def sparse():
                        t0 = time.perf_counter()
                        eng.fill_sparse_dev(*args, go, a.tile, hr.data_ptr(), hc.data_ptr())
                        eng.sync()
                        t1 = time.perf_counter()
                        tr = eng.trace_sparse_dev(*args, go, geom, hr.data_ptr(), hc.data_ptr())
                        t2 = time.perf_counter()
                        return tr, {"fill_ms": (t1 - t0) * 1e3, "trace_ms": (t2 - t1) * 1e3}

                    tr, pms = timed(sparse)
                    edit = tr[1].replace("\0", "")
                    row.update({"sparse_call_ms": round(pms["call_ms"][0], 3), "sparse_call_ms_spread": round(pms["call_ms"][1], 3),
                                "sparse_fill_ms": round(pms["fill_ms"][0], 3), "sparse_trace_ms": round(pms["trace_ms"][0], 3),
                                "sparse_cost_equal": int(tr[2] == res["score"]), "sparse_string_equal": int(edit == res["cigar"])})
                    del hr, hc
                rows.append(row)
            del ty, tx

    lines = []
    lines.append("related pairs n x n (15 %% substitutions, 2 %% indels), BLOSUM62, device-resident; one untimed pass, "
                 "then %d timed: medians (spread = max - min)" % a.repeats)
    lines.append("align = Engine.align_pair_dev (score in one direction + fill + walk); score_dev = Engine.score_dev "
                 "(split from both ends where it applies); every CIGAR replayed on the host: score and end cell equal")
    lines.append("mode       n   TR strips chunks codes MiB   moves | align call ms (spread)  score ms   fill ms (spread)   walk ms (spread) "
                 "fill GCUPS | score_dev call ms (spread) kernel ms  both ends | align/score")
    for r in rows:
        lines.append(f"{r['mode']:6s} {r['n']:6d} {r['strip_rows']:4d} {r['strips']:6d} {r['chunks']:6d} {r['code_mib']:9.1f} {r['moves']:7d} | "
                     f"{r['align_call_ms']:13.3f} ({r['align_call_ms_spread']:6.3f}) {r['align_score_ms']:9.3f} "
                     f"{r['align_fill_ms']:9.3f} ({r['align_fill_ms_spread']:6.3f}) {r['align_walk_ms']:9.3f} "
                     f"({r['align_walk_ms_spread']:6.3f}) {r['fill_gcups']:10.1f} | {r['score_call_ms']:17.3f} "
                     f"({r['score_call_ms_spread']:6.3f}) {r['score_kernel_ms']:9.3f} {r['score_dev_both_ends']:10d} | "
                     f"{r['align_over_score']:11.2f}")
    lines.append("")
    lines.append("NW-LG beside the sparse fill (tileBx %d) + device Trace2 on the same pair (host clock; Trace2 moves to the "
                 "largest neighbour, diagonal first, which is another rule than \"the source of H, diagonal, F, E\"):" % a.tile)
    lines.append("     n  align call ms  sparse fill + trace ms (spread)   fill ms  trace ms  cost equal  string equal")
    for r in rows:
        if "sparse_call_ms" in r:
            lines.append(f"{r['n']:6d} {r['align_call_ms']:14.3f} {r['sparse_call_ms']:23.3f} ({r['sparse_call_ms_spread']:6.3f}) "
                         f"{r['sparse_fill_ms']:9.3f} {r['sparse_trace_ms']:9.3f} {r['sparse_cost_equal']:11d} "
                         f"{r['sparse_string_equal']:13d}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps({"tool": "align_pair_bench", "sizes": a.sizes, "repeats": a.repeats, "rows": rows}), flush=True)


if __name__ == "__main__":
    main()
