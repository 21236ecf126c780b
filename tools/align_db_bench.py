"""Alignments of the best hits of a database search against the search that found them.

Workload (seeded, that of tools/score_db_bench.py): one query of 375 letters against 32 768 subjects
whose lengths are log-normal (median 300, sigma 0.6), clipped to 40..2000; alphabet 20, BLOSUM62;
SW-AG -11/-1, SW-LG -11/-11 and NW-AG -11/-1.  Everything device-resident.  Per mode:
Engine.score_db_dev over the whole database, then Engine.align_db_dev on the top 128, 1024 and 8192
subjects by score (equal scores: the smaller index first).

Per variant one untimed pass, then --repeats timed passes; host clock around the synchronous calls and
the hipEvent times the calls report (the search's kernels; the fill and the walk launches of the
alignment, summed over its chunks); medians.  The fill's cell rate (real cells: query letters x subject
letters of the hits) stands next to the score kernel's on the same hits: the hits copied into a
database of their own and run through score_db_dev.  Every hit's score and end cell are compared with
the search's entry, and the first --verify hits of every list with tests/_align_oracle.py, exactly.
Prints a table and one JSON line."""
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

from tools.score_db_bench import MODES, make_db  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--subjects", type=int, default=32768)
    ap.add_argument("--query", type=int, default=375)
    ap.add_argument("--tops", type=int, nargs="*", default=[128, 1024, 8192])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--verify", type=int, default=32)
    a = ap.parse_args()

    import torch
    import gpuseqalign_amd as gsa
    from gpuseqalign_amd import formats as F
    from tests import _align_oracle as ao

    assert torch.cuda.is_available(), "needs cuda:0"
    dev = torch.device("cuda:0")
    sub = F.read_subst_json(os.path.join(ROOT, "tests", "golden", "resrc", "subst.json")).matrix("blosum62")
    substsz = int(round(sub.size ** 0.5))
    ts = torch.from_numpy(sub.ravel().copy()).to(dev)
    rng = np.random.default_rng(2024)
    query = np.concatenate([[0], rng.integers(0, 20, a.query)]).astype(np.int32)
    tq = torch.from_numpy(query).to(dev)
    lens = np.clip(np.rint(np.exp(rng.normal(np.log(300.0), 0.6, a.subjects))), 40, 2000).astype(np.int64)
    db, off = make_db(lens, 7)
    tdb = torch.from_numpy(db).to(dev)
    torch.cuda.synchronize(dev)

    def timed(fn):
        """fn -> (value, dict of ms); one untimed pass, then the medians of the timed ones."""
        acc = {}
        val = None
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
        return val, {k: statistics.median(v) for k, v in acc.items()}

    rows = []
    with gsa.Engine(0) as eng:
        for name, go, ge, local in MODES:
            def search():
                r = eng.score_db_dev(tq.data_ptr(), len(query), tdb.data_ptr(), off, ts.data_ptr(), substsz, go, ge, local)
                return r, {"kernel_ms": r[0]["kernel_ms"]}

            scores, sms = timed(search)
            assert eng.last_launch()["kind"] == "score_lanes"
            order = sorted(range(a.subjects), key=lambda s: (-scores[s]["score"], s))
            for top in a.tops:
                hits = order[:top]

                def align():
                    r = eng.align_db_dev(tq.data_ptr(), len(query), tdb.data_ptr(), off, hits, ts.data_ptr(), substsz, go,
                                         ge, local)
                    info = eng.last_align_db_info()
                    align.info = info
                    return r, {"fill_ms": info["fill_ms"], "walk_ms": info["walk_ms"]}

                res, ams = timed(align)
                info = align.info
                assert info["lane_hits"] == len(hits) and info["unsupported"] == 0, info
                for s, r in zip(hits, res):
                    assert r["status"] == 0
                    assert (r["score"], r["i_end"], r["j_end"]) == (scores[s]["score"], scores[s]["i_end"], scores[s]["j_end"])
                for s, r in list(zip(hits, res))[:a.verify]:
                    want = ao.align(query, db[off[s]:off[s + 1]], sub, go, ge, local)
                    got = (r["score"], r["i_start"], r["j_start"], r["i_end"], r["j_end"], r["cigar"])
                    assert got == want, (name, s, got, want)
                # the same hits as a database of their own through the score kernel
                hdb, hoff = [], [0]
                for s in hits:
                    hdb.append(db[off[s]:off[s + 1]])
                    hoff.append(hoff[-1] + len(hdb[-1]))
                thits = torch.from_numpy(np.concatenate(hdb)).to(dev)
                torch.cuda.synchronize(dev)
                hoff = np.asarray(hoff, np.int64)

                def score_hits():
                    r = eng.score_db_dev(tq.data_ptr(), len(query), thits.data_ptr(), hoff, ts.data_ptr(), substsz, go, ge,
                                         local)
                    return r, {"kernel_ms": r[0]["kernel_ms"]}

                _, hms = timed(score_hits)
                assert eng.last_launch()["kind"] == "score_lanes" and eng.last_launch()["npairs"] == len(hits)
                cells = int(sum(int(lens[s]) for s in hits)) * a.query
                rows.append({"mode": name, "top": top, "letters": int(sum(int(lens[s]) for s in hits)),
                             "search_ms": round(sms["call_ms"], 3), "search_kernel_ms": round(sms["kernel_ms"], 3),
                             "align_ms": round(ams["call_ms"], 3), "fill_ms": round(ams["fill_ms"], 3),
                             "walk_ms": round(ams["walk_ms"], 3), "chunks": info["chunks"], "tasks": info["tasks"],
                             "code_mib": round(info["code_bytes"] / 2 ** 20, 1),
                             "score_hits_kernel_ms": round(hms["kernel_ms"], 3),
                             "fill_gcups": round(cells / ams["fill_ms"] / 1e6, 1),
                             "score_hits_gcups": round(cells / hms["kernel_ms"] / 1e6, 1),
                             "align_over_search": round(ams["call_ms"] / sms["call_ms"], 2),
                             "kernels_over_search_kernels": round((ams["fill_ms"] + ams["walk_ms"]) / sms["kernel_ms"], 2)})
                del thits

    print("query %d letters, %d subjects (log-normal, median 300, sigma 0.6, clipped 40..2000; %d letters); "
          "%d timed passes, medians; the first %d hits of every list equal the oracle's alignments"
          % (a.query, a.subjects, int(lens.sum()), a.repeats, a.verify))
    print("mode    top   hit letters  search ms (kernels)   align ms   fill ms   walk ms  chunks  codes MiB  "
          "score-kernel ms on the hits   fill GCUPS  score GCUPS  align/search  (kernels)")
    for r in rows:
        print(f"{r['mode']:6s} {r['top']:5d} {r['letters']:12d} {r['search_ms']:10.3f} ({r['search_kernel_ms']:7.3f}) "
              f"{r['align_ms']:10.3f} {r['fill_ms']:9.3f} {r['walk_ms']:9.3f} {r['chunks']:7d} {r['code_mib']:10.1f} "
              f"{r['score_hits_kernel_ms']:28.3f} {r['fill_gcups']:12.1f} {r['score_hits_gcups']:12.1f} "
              f"{r['align_over_search']:13.2f} {r['kernels_over_search_kernels']:10.2f}")
    print(json.dumps({"tool": "align_db_bench", "query": a.query, "subjects": a.subjects, "repeats": a.repeats,
                      "verified_per_list": a.verify, "rows": rows}), flush=True)


if __name__ == "__main__":
    main()
