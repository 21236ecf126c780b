"""Database search against the batched K-rows path.

Workload (seeded): one query of 375 letters against 32 768 subjects whose lengths are log-normal
(median 300, sigma 0.6), clipped to 40..2000; alphabet 20, BLOSUM62; SW-AG -11/-1, SW-LG -11/-11 and
NW-AG -11/-1.  Everything device-resident.  Engine.score_db_dev (subjects up to Lmax on the lane
kernel, nw_lanes.hip) against the parent's way of doing the job, Engine.score_batch_dev over the same
pairs in the same process, and against score_db_dev with GSA_DB_LANES=0 (the same K-rows path behind
the same entry point).

Length sweep: 4096 subjects, all of one length, at 64 ... 4096: the lane kernel forced for every
subject (GSA_DB_MAXC=8191) against GSA_DB_LANES=0.  Lmax is the largest swept length at which the
lane kernel still wins in all three modes.

Per variant one untimed pass, then --repeats timed passes taken in turn (the variants alternate),
host clock around the synchronous calls and the hipEvent time of each call's kernels; medians of
both.  The garbage collector is off inside a timed call (a call returns tens of thousands of dicts).
Every result is compared between the paths.  GCUPS count
real cells (query letters x subject letters).  Prints tables and one JSON line."""
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
    """Subjects of the given lengths back to back, each with its header 0; the offsets."""
    rng = np.random.default_rng(seed)
    off = np.concatenate([[0], np.cumsum(np.asarray(lens, np.int64) + 1)]).astype(np.int64)
    db = rng.integers(0, 20, int(off[-1])).astype(np.int32)
    db[off[:-1]] = 0
    return db, off


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--subjects", type=int, default=32768)
    ap.add_argument("--query", type=int, default=375)
    ap.add_argument("--sweep", type=int, nargs="*", default=[64, 128, 256, 512, 1024, 2048, 4096])
    ap.add_argument("--sweep-subjects", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()

    import torch
    import gpuseqalign_amd as gsa
    from gpuseqalign_amd import formats as F

    assert torch.cuda.is_available(), "needs cuda:0"
    dev = torch.device("cuda:0")
    sub = F.read_subst_json(os.path.join(ROOT, "tests", "golden", "resrc", "subst.json")).matrix("blosum62")
    substsz = int(round(sub.size ** 0.5))
    ts = torch.from_numpy(sub.ravel().copy()).to(dev)
    rng = np.random.default_rng(2024)
    query = np.concatenate([[0], rng.integers(0, 20, a.query)]).astype(np.int32)
    tq = torch.from_numpy(query).to(dev)

    def alternate(variants):
        """{name: fn -> (seconds, kernel_ms, results)}: medians over the timed passes; results equal."""
        times = {v: [] for v in variants}
        kms = {v: [] for v in variants}
        got = {}
        for it in range(1 + a.repeats):  # pass 0: warm-up
            for v, fn in variants.items():
                gc.collect()
                gc.disable()  # a call returns tens of thousands of dicts: no collection inside the timed part
                try:
                    dt, k, got[v] = fn()
                finally:
                    gc.enable()
                if it:
                    times[v].append(dt)
                    kms[v].append(k)
        first = next(iter(variants))
        for v in variants:
            assert got[v] == got[first], "results differ: %s against %s" % (v, first)
        return ({v: statistics.median(t) for v, t in times.items()}, {v: statistics.median(k) for v, k in kms.items()})

    rows, sweep_rows = [], []
    with gsa.Engine(0) as eng:
        def run_db(db_t, off, go, ge, local, lanes, maxc=None):
            eng.set_knob("GSA_DB_LANES", None if lanes else "0")
            eng.set_knob("GSA_DB_MAXC", maxc)
            t0 = time.perf_counter()
            r = eng.score_db_dev(tq.data_ptr(), len(query), db_t.data_ptr(), off, ts.data_ptr(), substsz, go, ge, local)
            dt = time.perf_counter() - t0
            eng.set_knob("GSA_DB_LANES", None)
            eng.set_knob("GSA_DB_MAXC", None)
            return dt, r[0]["kernel_ms"], [(d["score"], d["i_end"], d["j_end"]) for d in r]

        # the workload
        lens = np.clip(np.rint(np.exp(rng.normal(np.log(300.0), 0.6, a.subjects))), 40, 2000).astype(np.int64)
        db, off = make_db(lens, 7)
        tdb = torch.from_numpy(db).to(dev)
        torch.cuda.synchronize(dev)
        cells = int(lens.sum()) * a.query
        ptrs = [(tq.data_ptr(), len(query), tdb.data_ptr() + 4 * int(off[s]), int(off[s + 1] - off[s]))
                for s in range(a.subjects)]
        for name, go, ge, local in MODES:
            def batch():
                t0 = time.perf_counter()
                r = eng.score_batch_dev(ptrs, ts.data_ptr(), substsz, go, ge, local)
                dt = time.perf_counter() - t0
                assert eng.last_launch()["kind"] == "score_krow"
                return dt, r[0]["kernel_ms"], [(d["score"], d["i_end"], d["j_end"]) for d in r]

            def lanes():
                out = run_db(tdb, off, go, ge, local, True)
                ll = eng.last_launch()
                assert ll["kind"] == "score_lanes", ll
                lanes.npairs = ll["npairs"]
                return out

            med, kms = alternate({"score_batch_dev": batch, "score_db_dev": lanes,
                                  "score_db_dev LANES=0": lambda: run_db(tdb, off, go, ge, local, False)})
            for v in med:
                rows.append({"mode": name, "variant": v, "ms": round(med[v] * 1e3, 3), "kernel_ms": round(kms[v], 3),
                             "gcups": round(cells / med[v] / 1e9, 1), "kernel_gcups": round(cells / kms[v] / 1e6, 1),
                             "batch_over_this": round(med["score_batch_dev"] / med[v], 2),
                             "kernel_batch_over_this": round(kms["score_batch_dev"] / kms[v], 2),
                             "lane_subjects": lanes.npairs if v == "score_db_dev" else 0})
        del tdb

        # the length sweep
        for L in a.sweep:
            db, off = make_db([L] * a.sweep_subjects, 100 + L)
            tdb = torch.from_numpy(db).to(dev)
            torch.cuda.synchronize(dev)
            cells = a.sweep_subjects * L * a.query
            for name, go, ge, local in MODES:
                def forced():
                    out = run_db(tdb, off, go, ge, local, True, "8191")
                    ll = eng.last_launch()
                    assert ll["kind"] == "score_lanes" and ll["npairs"] == a.sweep_subjects, ll
                    return out

                med, kms = alternate({"lanes": forced, "krow": lambda: run_db(tdb, off, go, ge, local, False)})
                sweep_rows.append({"length": L, "mode": name, "lanes_ms": round(med["lanes"] * 1e3, 3),
                                   "krow_ms": round(med["krow"] * 1e3, 3),
                                   "lanes_kernel_ms": round(kms["lanes"], 3), "krow_kernel_ms": round(kms["krow"], 3),
                                   "lanes_gcups": round(cells / med["lanes"] / 1e9, 1),
                                   "krow_gcups": round(cells / med["krow"] / 1e9, 1),
                                   "krow_over_lanes": round(med["krow"] / med["lanes"], 2)})
            del tdb

    print("query %d letters, %d subjects (log-normal, median 300, sigma 0.6, clipped 40..2000; %d letters)"
          % (a.query, a.subjects, int(lens.sum())))
    print("mode   variant                 ms (host)   kernel ms     GCUPS  kernel GCUPS  batch/this  (kernel)  on lanes")
    for r in rows:
        print(f"{r['mode']:6s} {r['variant']:22s} {r['ms']:10.3f} {r['kernel_ms']:11.3f} {r['gcups']:9.1f} "
              f"{r['kernel_gcups']:13.1f} {r['batch_over_this']:11.2f} {r['kernel_batch_over_this']:9.2f} "
              f"{r['lane_subjects']:9d}")
    print()
    print("length sweep: %d subjects of one length, lane kernel forced (GSA_DB_MAXC=8191) against GSA_DB_LANES=0"
          % a.sweep_subjects)
    print("length mode    lanes ms (kernel)      krow ms (kernel)   lanes GCUPS  krow GCUPS  krow/lanes")
    for r in sweep_rows:
        print(f"{r['length']:6d} {r['mode']:6s} {r['lanes_ms']:9.3f} ({r['lanes_kernel_ms']:8.3f}) {r['krow_ms']:11.3f} "
              f"({r['krow_kernel_ms']:8.3f}) {r['lanes_gcups']:12.1f} {r['krow_gcups']:11.1f} {r['krow_over_lanes']:11.2f}")
    wins = [L for L in a.sweep if all(r["krow_over_lanes"] > 1.0 for r in sweep_rows if r["length"] == L)]
    print("lane kernel wins in all three modes at:", wins)
    print(json.dumps({"tool": "score_db_bench", "query": a.query, "subjects": a.subjects, "repeats": a.repeats,
                      "results_equal": True, "rows": rows, "sweep": sweep_rows, "lanes_win_at": wins}), flush=True)


if __name__ == "__main__":
    main()
