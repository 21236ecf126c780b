"""Overlap (dovetail) database search beside the semi-global and the global shape.

Workload B of 2.2f (seeded): --queries queries of 100..1000 letters against --subjects subjects whose
lengths are 2.2d's log-normal (median 300, sigma 0.6, clipped to 40..2000), the best --top of every
query; alphabet 20, BLOSUM62, everything device-resident; an affine (-11 / -1) and a linear
(-11 / -11) gap model.

Scores: Engine.score_db_overlap_dev beside Engine.score_db_semi_dev -- the yardstick: the same
schedule, layout and per-cell code, without the fold on column C and the 16-lane reduction -- and
beside Engine.score_db_multi_dev global.  Alignments: for the best --atop subjects of every query by
the overlap score, Engine.align_db_overlap_dev beside Engine.align_db_semi_dev and
Engine.align_db_multi_dev global on the same hits.

2.2d's method: all sides in the same process, one untimed pass each, then --repeats timed passes
taken in turn; the hipEvent times the calls report (lanes_ms; fill_ms + walk_ms) and the host clock
around the synchronous calls; medians, with the spread.  The overlap results are compared with
tests/_overlap_oracle.py on a sample in every run.  Progress goes to stderr.  Prints tables and one
JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.score_db_multi_bench import lognormal_lens, make_db  # noqa: E402

GAPS = [("AG", -11, -1), ("LG", -11, -11)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=64)
    ap.add_argument("--subjects", type=int, default=32768)
    ap.add_argument("--top", type=int, default=100)
    ap.add_argument("--atop", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--sample", type=int, default=48, help="pairs compared with the oracle per gap model")
    a = ap.parse_args()

    import torch
    import gpuseqalign_amd as gsa
    from gpuseqalign_amd import formats as F
    from tests import _overlap_oracle as oo

    assert torch.cuda.is_available(), "needs cuda:0"
    dev = torch.device("cuda:0")
    sub = F.read_subst_json(os.path.join(ROOT, "tests", "golden", "resrc", "subst.json")).matrix("blosum62")
    substsz = int(round(sub.size ** 0.5))
    ts = torch.from_numpy(sub.ravel().copy()).to(dev)
    rng = np.random.default_rng(2024)
    lognormal_lens(rng, 4096)  # workload A's draw: the same generator state as tools/score_db_multi_bench.py
    slens = lognormal_lens(rng, a.subjects)
    qlens = rng.integers(100, 1001, a.queries)
    db, off = make_db(slens, 8)
    qs, qoff = make_db(qlens, 9)
    tdb, tq = torch.from_numpy(db).to(dev), torch.from_numpy(qs).to(dev)
    torch.cuda.synchronize(dev)
    cells = int(slens.sum()) * int(qlens.sum())
    seq = lambda buf, o, k: buf[int(o[k]):int(o[k + 1])]
    score_rows, align_rows = [], []
    ptrs = (tq.data_ptr(), qoff, tdb.data_ptr(), off)

    with gsa.Engine(0) as eng:
        def score(side, go, ge):
            t0 = time.perf_counter()
            if side == "global":
                r = eng.score_db_multi_dev(*ptrs, ts.data_ptr(), substsz, go, ge, False, top=a.top, want_scores=False)
                info = eng.last_score_db_multi_info()
            else:
                r = getattr(eng, "score_db_%s_dev" % side)(*ptrs, ts.data_ptr(), substsz, go, ge, top=a.top,
                                                           want_scores=False)
                info = getattr(eng, "last_score_db_%s_info" % side)()
            return time.perf_counter() - t0, r, info

        def align(side, hq, hs, go, ge):
            t0 = time.perf_counter()
            if side == "global":
                r = eng.align_db_multi_dev(*ptrs, hq, hs, ts.data_ptr(), substsz, go, ge, False)
                info = eng.last_align_db_multi_info()
            else:
                r = getattr(eng, "align_db_%s_dev" % side)(*ptrs, hq, hs, ts.data_ptr(), substsz, go, ge)
                info = getattr(eng, "last_align_db_%s_info" % side)()
            return time.perf_counter() - t0, r, info

        for name, go, ge in GAPS:
            sides = ("global", "semi", "overlap")
            call, lanes, sel, last = ({s: [] for s in sides} for _ in range(4))
            for it in range(1 + a.repeats):  # pass 0: warm-up
                for s in sides:
                    dt, r, info = score(s, go, ge)
                    assert info["other_queries"] == 0 and info["lane_queries"] == a.queries, (s, info)
                    last[s] = (r, info)
                    if it:
                        call[s].append(dt * 1e3)
                        lanes[s].append(info["lanes_ms"])
                        sel[s].append(info["select_ms"])
                print("scores %s pass %d: %s" % (name, it, {s: round(last[s][1]["lanes_ms"], 3) for s in sides}),
                      file=sys.stderr, flush=True)
            hits = last["overlap"][0]["hits"]
            # the oracle on a sample: ranks 0, top / 2 and top - 1 of queries spread over the set
            picks = [(q, k) for q in np.linspace(0, a.queries - 1, max(a.sample // 3, 1)).astype(int)
                     for k in (0, hits.shape[1] // 2, hits.shape[1] - 1)]
            on_col = 0
            for q, k in picks:
                h = hits[q][k]
                want = oo.score(seq(qs, qoff, q), seq(db, off, int(h["subject"])), sub, go, ge)
                assert (int(h["score"]), int(h["i_end"]), int(h["j_end"])) == want, (name, q, k, h, want)
                on_col += int(want[1] < int(qlens[q]))
            for s in sides:
                score_rows.append({"gaps": name, "side": s, "lanes_ms": round(statistics.median(lanes[s]), 3),
                                   "lanes_spread": [round(min(lanes[s]), 3), round(max(lanes[s]), 3)],
                                   "select_ms": round(statistics.median(sel[s]), 3),
                                   "call_ms": round(statistics.median(call[s]), 2),
                                   "tcups": round(cells / statistics.median(lanes[s]) / 1e9, 2),
                                   "launches": last[s][1]["launches"], "units": last[s][1]["units"],
                                   "profile_builds": last[s][1]["profile_builds"]})
            score_rows[-1]["sample_ends_on_column_C"] = [on_col, len(picks)]

            hq = np.repeat(np.arange(a.queries, dtype=np.int32), a.atop)
            hs = np.ascontiguousarray(hits["subject"][:, :a.atop], dtype=np.int32).ravel()
            acall, fill, walk, alast = ({s: [] for s in sides} for _ in range(4))
            for it in range(1 + a.repeats):
                for s in sides:
                    dt, r, info = align(s, hq, hs, go, ge)
                    assert info["unsupported"] == 0 and info["lane_hits"] == len(hq), (s, info)
                    alast[s] = (r, info)
                    if it:
                        acall[s].append(dt * 1e3)
                        fill[s].append(info["fill_ms"])
                        walk[s].append(info["walk_ms"])
                print("alignments %s pass %d: %s" % (name, it, {s: round(alast[s][1]["fill_ms"] + alast[s][1]["walk_ms"], 3)
                                                               for s in sides}), file=sys.stderr, flush=True)
            res = alast["overlap"][0]
            for h in np.linspace(0, len(hq) - 1, max(a.sample // 3, 1)).astype(int):
                pair = (seq(qs, qoff, int(hq[h])), seq(db, off, int(hs[h])))
                want = oo.align(*pair, sub, go, ge)
                got = tuple(res[h][f] for f in ("score", "i_start", "j_start", "i_end", "j_end", "cigar"))
                assert res[h]["status"] == 0 and got == want, (name, h, got, want)
                assert oo.replay(*pair, sub, go, ge, got) == got[0], (name, h)
            for s in sides:
                fw = [f + w for f, w in zip(fill[s], walk[s])]
                align_rows.append({"gaps": name, "side": s, "hits": len(hq), "fill_ms": round(statistics.median(fill[s]), 3),
                                   "walk_ms": round(statistics.median(walk[s]), 3),
                                   "fill_walk_ms": round(statistics.median(fw), 3),
                                   "fill_walk_spread": [round(min(fw), 3), round(max(fw), 3)],
                                   "call_ms": round(statistics.median(acall[s]), 2),
                                   "code_bytes": alast[s][1]["code_bytes"], "chunks": alast[s][1]["chunks"],
                                   "launches": alast[s][1]["launches"]})

    print("workload B: %d queries of 100..1000 letters x %d subjects, top %d; medians of %d passes taken in turn, (min ... max)"
          % (a.queries, a.subjects, a.top, a.repeats))
    print("gaps  side    lanes ms (spread)               select ms   call ms   TCUPS  launches    units   builds")
    for r in score_rows:
        print(f"{r['gaps']:5s} {r['side']:7s} {r['lanes_ms']:8.3f} ({r['lanes_spread'][0]:8.3f} ... {r['lanes_spread'][1]:8.3f}) "
              f"{r['select_ms']:10.3f} {r['call_ms']:9.2f} {r['tcups']:7.2f} {r['launches']:9d} {r['units']:8d} {r['profile_builds']:8d}")
    for name, _, _ in GAPS:
        by = {r["side"]: r["lanes_ms"] for r in score_rows if r["gaps"] == name}
        print("%s lanes_ms overlap / semi %.3f, overlap / global %.3f" % (name, by["overlap"] / by["semi"], by["overlap"] / by["global"]))
    print("alignments of the best %d subjects of every query by the overlap score, the same hits on all sides" % a.atop)
    print("gaps  side     hits   fill ms   walk ms  fill + walk ms (spread)           call ms   code bytes  chunks  launches")
    for r in align_rows:
        print(f"{r['gaps']:5s} {r['side']:7s} {r['hits']:5d} {r['fill_ms']:9.3f} {r['walk_ms']:9.3f} {r['fill_walk_ms']:9.3f} "
              f"({r['fill_walk_spread'][0]:8.3f} ... {r['fill_walk_spread'][1]:8.3f}) {r['call_ms']:9.2f} {r['code_bytes']:12d} "
              f"{r['chunks']:7d} {r['launches']:9d}")
    for name, _, _ in GAPS:
        by = {r["side"]: r["fill_walk_ms"] for r in align_rows if r["gaps"] == name}
        print("%s fill + walk overlap / semi %.3f, overlap / global %.3f" % (name, by["overlap"] / by["semi"], by["overlap"] / by["global"]))
    print(json.dumps({"tool": "score_db_overlap_bench", "queries": a.queries, "subjects": a.subjects, "top": a.top,
                      "atop": a.atop, "repeats": a.repeats, "oracle_sample_equal": True, "scores": score_rows,
                      "alignments": align_rows}), flush=True)


if __name__ == "__main__":
    main()
