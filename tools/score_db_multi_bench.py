"""Many queries against one database: Engine.score_db_multi_dev against the parent's way, a loop of
Engine.score_db_dev over the queries.

Workload A (seeded): all-vs-all of --seqs sequences whose lengths are 2.2d's log-normal (median 300,
sigma 0.6), clipped to 40..2000; scores only; SW-AG -11/-1, SW-LG -11/-11 and NW-AG -11/-1.
Workload B: --queries queries of 100..1000 letters against 2.2d's --subjects subjects, the best
--top of every query (the loop's hits: a host sort of its scores, outside the timed part).
Alphabet 20, BLOSUM62, everything device-resident.

2.2d's method: both ways in the same process, one untimed pass each, then --repeats timed passes
taken in turn; host clock around the synchronous calls (the loop: summed over its calls) and the
hipEvent time of the kernels (the loop: summed over its calls); medians, and the spread (min ... max)
of the kernel times, which is what the multi call's kernel time is held against.  Every result is
compared between the two ways in every pass.  GCUPS count real cells (query letters x subject
letters) over the call time.

The unit size is a compile-time constant of the library: --lib PATH measures another build in a run
of its own (make -B with DBM_UNIT=n and OUT=../libgsa_uN.so, then make -B again for the tree's
library).  Progress goes to stderr.  Prints tables and one JSON line."""
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

MODES = [("SW-AG", -11, -1, True), ("SW-LG", -11, -11, True), ("NW-AG", -11, -1, False)]


def make_db(lens, seed):
    """Sequences of the given lengths back to back, each with its header 0; the offsets."""
    rng = np.random.default_rng(seed)
    off = np.concatenate([[0], np.cumsum(np.asarray(lens, np.int64) + 1)]).astype(np.int64)
    db = rng.integers(0, 20, int(off[-1])).astype(np.int32)
    db[off[:-1]] = 0
    return db, off


def lognormal_lens(rng, n):
    return np.clip(np.rint(np.exp(rng.normal(np.log(300.0), 0.6, n))), 40, 2000).astype(np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seqs", type=int, default=4096)
    ap.add_argument("--queries", type=int, default=64)
    ap.add_argument("--subjects", type=int, default=32768)
    ap.add_argument("--top", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--lib", default=None, help="another build of libgsa.so (another unit size)")
    a = ap.parse_args()
    if a.lib:
        os.environ["GSA_LIB"] = os.path.abspath(a.lib)

    import torch
    import gpuseqalign_amd as gsa
    from gpuseqalign_amd import formats as F

    assert torch.cuda.is_available(), "needs cuda:0"
    dev = torch.device("cuda:0")
    sub = F.read_subst_json(os.path.join(ROOT, "tests", "golden", "resrc", "subst.json")).matrix("blosum62")
    substsz = int(round(sub.size ** 0.5))
    ts = torch.from_numpy(sub.ravel().copy()).to(dev)
    unit = gsa.score_db_multi_unit()
    rows = []

    with gsa.Engine(0) as eng:
        def loop_way(tq, qoff, tdb, off, go, ge, local, cells):
            """(seconds, kernel ms, [nq, nsubj, 3]) of score_db_dev per query; the clock runs inside the calls
            only.  `cells`: the end cells too (else the scores alone, column 0)."""
            nq, n = len(qoff) - 1, len(off) - 1
            out = np.zeros((nq, n, 3), np.int32)
            dt = kms = 0.0
            for q in range(nq):
                t0 = time.perf_counter()
                r = eng.score_db_dev(tq.data_ptr() + 4 * int(qoff[q]), int(qoff[q + 1] - qoff[q]), tdb.data_ptr(), off,
                                     ts.data_ptr(), substsz, go, ge, local)
                dt += time.perf_counter() - t0
                kms += r[0]["kernel_ms"]
                if cells:
                    out[q] = [(d["score"], d["i_end"], d["j_end"]) for d in r]
                else:
                    out[q, :, 0] = np.fromiter((d["score"] for d in r), np.int32, n)
            return dt, kms, out

        def multi_way(tq, qoff, tdb, off, go, ge, local, top):
            t0 = time.perf_counter()
            r = eng.score_db_multi_dev(tq.data_ptr(), qoff, tdb.data_ptr(), off, ts.data_ptr(), substsz, go, ge, local,
                                       top=top, want_scores=top == 0)
            dt = time.perf_counter() - t0
            return dt, r["kernel_ms"], r, eng.last_score_db_multi_info()

        def measure(workload, tq, qoff, tdb, off, cells, top):
            for name, go, ge, local in MODES:
                t = {"loop": [], "multi": []}
                k = {"loop": [], "multi": []}
                info = None
                for it in range(1 + a.repeats):  # pass 0: warm-up
                    gc.collect()
                    gc.disable()  # the loop's calls return thousands of dicts each: no collection inside a pass
                    try:
                        dl, kl, ref = loop_way(tq, qoff, tdb, off, go, ge, local, top > 0)
                        dm, km, r, info = multi_way(tq, qoff, tdb, off, go, ge, local, top)
                    finally:
                        gc.enable()
                    if top == 0:
                        assert np.array_equal(r["scores"], ref[:, :, 0]), "scores differ: %s %s" % (workload, name)
                    else:
                        n = ref.shape[1]
                        for q in range(ref.shape[0]):
                            order = np.lexsort((np.arange(n), -ref[q, :, 0].astype(np.int64)))[:top]
                            h = r["hits"][q]
                            assert np.array_equal(h["subject"], order) and np.array_equal(h["score"], ref[q, order, 0]) and \
                                np.array_equal(h["i_end"], ref[q, order, 1]) and np.array_equal(h["j_end"], ref[q, order, 2]), \
                                "hits differ: %s %s query %d" % (workload, name, q)
                    if it:
                        t["loop"].append(dl)
                        t["multi"].append(dm)
                        k["loop"].append(kl)
                        k["multi"].append(km)
                    print("%s %s pass %d: loop %.1f ms, multi %.1f ms" % (workload, name, it, dl * 1e3, dm * 1e3),
                          file=sys.stderr, flush=True)
                med = {v: statistics.median(t[v]) for v in t}
                kmed = {v: statistics.median(k[v]) for v in k}
                rows.append({"workload": workload, "mode": name, "unit": unit,
                             "loop_ms": round(med["loop"] * 1e3, 2), "multi_ms": round(med["multi"] * 1e3, 2),
                             "loop_over_multi": round(med["loop"] / med["multi"], 2),
                             "loop_kernel_ms": round(kmed["loop"], 3), "multi_kernel_ms": round(kmed["multi"], 3),
                             "loop_kernel_spread": [round(min(k["loop"]), 3), round(max(k["loop"]), 3)],
                             "multi_kernel_spread": [round(min(k["multi"]), 3), round(max(k["multi"]), 3)],
                             "kernel_multi_over_loop": round(kmed["multi"] / kmed["loop"], 4),
                             "lanes_ms": round(info["lanes_ms"], 3), "select_ms": round(info["select_ms"], 3),
                             "profile_builds": info["profile_builds"], "units": info["units"],
                             "launches": info["launches"], "workgroups": info["workgroups"],
                             "loop_gcups": round(cells / med["loop"] / 1e9, 1),
                             "multi_gcups": round(cells / med["multi"] / 1e9, 1)})

        rng = np.random.default_rng(2024)
        # A: all-vs-all
        lens = lognormal_lens(rng, a.seqs)
        db, off = make_db(lens, 7)
        tdb = torch.from_numpy(db).to(dev)
        torch.cuda.synchronize(dev)
        measure("A all-vs-all %d" % a.seqs, tdb, off, tdb, off, int(lens.sum()) ** 2, 0)
        del tdb
        # B: a set of queries against a database, the best of every query
        slens = lognormal_lens(rng, a.subjects)
        qlens = rng.integers(100, 1001, a.queries)
        db, off = make_db(slens, 8)
        qs, qoff = make_db(qlens, 9)
        tdb, tq = torch.from_numpy(db).to(dev), torch.from_numpy(qs).to(dev)
        torch.cuda.synchronize(dev)
        measure("B %d x %d top %d" % (a.queries, a.subjects, a.top), tq, qoff, tdb, off, int(slens.sum()) * int(qlens.sum()),
                a.top)

    print("unit size %d wave tasks (%s); medians of %d passes taken in turn; kernel ms with (min ... max)"
          % (unit, a.lib or "the tree's library", a.repeats))
    print("workload               mode    loop ms  multi ms  loop/multi   loop kernel ms (spread)       multi kernel ms (spread)"
          "    multi/loop  lanes ms  select ms   builds    units  loop GCUPS  multi GCUPS")
    for r in rows:
        print(f"{r['workload']:22s} {r['mode']:6s} {r['loop_ms']:9.2f} {r['multi_ms']:9.2f} {r['loop_over_multi']:10.2f} "
              f"{r['loop_kernel_ms']:10.3f} ({r['loop_kernel_spread'][0]:9.3f} ... {r['loop_kernel_spread'][1]:9.3f}) "
              f"{r['multi_kernel_ms']:10.3f} ({r['multi_kernel_spread'][0]:9.3f} ... {r['multi_kernel_spread'][1]:9.3f}) "
              f"{r['kernel_multi_over_loop']:10.4f} {r['lanes_ms']:9.3f} {r['select_ms']:10.3f} {r['profile_builds']:8d} "
              f"{r['units']:8d} {r['loop_gcups']:11.1f} {r['multi_gcups']:12.1f}")
    print(json.dumps({"tool": "score_db_multi_bench", "unit": unit, "seqs": a.seqs, "queries": a.queries,
                      "subjects": a.subjects, "top": a.top, "repeats": a.repeats, "results_equal": True, "rows": rows}),
          flush=True)


if __name__ == "__main__":
    main()
