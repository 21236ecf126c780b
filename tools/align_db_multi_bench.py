"""The alignments of many queries' hits: Engine.align_db_multi_dev against the parent's way, a loop of
Engine.align_db_dev per query on the same hits.

Workload: 2.2f's workload B (the same seeds and draws): --queries queries of 100..1000 letters against
--subjects subjects whose lengths are 2.2d's log-normal (median 300, sigma 0.6, clipped to 40..2000);
the hits are every query's best --top subjects (one score_db_multi_dev call per mode, outside the timed
part), with top = 10 and top = 100; SW-AG -11/-1, SW-LG -11/-11 and NW-AG -11/-1.  Alphabet 20,
BLOSUM62, everything device-resident.

2.2d's method: both ways in the same process, one untimed pass each, then --repeats timed passes taken
in turn; host clock around the synchronous calls (the loop: summed over its calls) and the hipEvent time
of the fill and walk kernels (fill_ms + walk_ms; the loop: summed over its calls); medians and the
spread (min ... max) of both.  Every result of the two ways is compared in every pass.

The unit size is a compile-time constant of the library: --lib PATH measures another build in a run of
its own (make -B with DBA_UNIT=n and OUT=../libgsa_aN.so, then make -B again for the tree's library).
Progress goes to stderr.  Prints a table and one JSON line."""
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
    ap.add_argument("--seqs", type=int, default=4096, help="2.2f's workload A: drawn first, not run")
    ap.add_argument("--queries", type=int, default=64)
    ap.add_argument("--subjects", type=int, default=32768)
    ap.add_argument("--tops", type=int, nargs="+", default=[10, 100])
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
    unit = gsa.align_db_multi_unit()
    rows = []

    rng = np.random.default_rng(2024)
    lognormal_lens(rng, a.seqs)  # workload A's draw
    slens = lognormal_lens(rng, a.subjects)
    qlens = rng.integers(100, 1001, a.queries)
    db, off = make_db(slens, 8)
    qs, qoff = make_db(qlens, 9)
    tdb, tq = torch.from_numpy(db).to(dev), torch.from_numpy(qs).to(dev)
    torch.cuda.synchronize(dev)
    strip = lambda res: [tuple(v for k, v in sorted(d.items()) if k != "kernel_ms") for d in res]

    with gsa.Engine(0) as eng:
        def loop_way(subjects, go, ge, local):
            """(seconds, fill + walk ms, results in hit order, chunks) of align_db_dev per query."""
            dt = kms = 0.0
            out, chunks = [], 0
            for q in range(a.queries):
                t0 = time.perf_counter()
                r = eng.align_db_dev(tq.data_ptr() + 4 * int(qoff[q]), int(qoff[q + 1] - qoff[q]), tdb.data_ptr(), off,
                                     subjects[q], ts.data_ptr(), substsz, go, ge, local)
                dt += time.perf_counter() - t0
                info = eng.last_align_db_info()
                kms += info["fill_ms"] + info["walk_ms"]
                chunks += info["chunks"]
                out += r
            return dt, kms, out, chunks

        def multi_way(hq, hs, go, ge, local):
            t0 = time.perf_counter()
            r = eng.align_db_multi_dev(tq.data_ptr(), qoff, tdb.data_ptr(), off, hq, hs, ts.data_ptr(), substsz, go, ge, local)
            dt = time.perf_counter() - t0
            info = eng.last_align_db_multi_info()
            return dt, info["fill_ms"] + info["walk_ms"], r, info

        for top in a.tops:
            for name, go, ge, local in MODES:
                hits = eng.score_db_multi_dev(tq.data_ptr(), qoff, tdb.data_ptr(), off, ts.data_ptr(), substsz, go, ge, local,
                                              top=top, want_scores=False)["hits"]
                subjects = np.ascontiguousarray(hits["subject"], dtype=np.int32)
                hq = np.repeat(np.arange(a.queries, dtype=np.int32), subjects.shape[1])
                hs = subjects.ravel()
                t = {"loop": [], "multi": []}
                k = {"loop": [], "multi": []}
                info, loop_chunks = None, 0
                for it in range(1 + a.repeats):  # pass 0: warm-up
                    gc.collect()
                    gc.disable()
                    try:
                        dl, kl, ref, loop_chunks = loop_way(subjects, go, ge, local)
                        dm, km, r, info = multi_way(hq, hs, go, ge, local)
                    finally:
                        gc.enable()
                    assert strip(r) == strip(ref), "results differ: top %d %s pass %d" % (top, name, it)
                    assert all(d["status"] == 0 for d in r), "a hit was not traced: top %d %s" % (top, name)
                    if it:
                        t["loop"].append(dl)
                        t["multi"].append(dm)
                        k["loop"].append(kl)
                        k["multi"].append(km)
                    print("top %d %s pass %d: loop %.2f ms, multi %.2f ms" % (top, name, it, dl * 1e3, dm * 1e3),
                          file=sys.stderr, flush=True)
                med = {v: statistics.median(t[v]) * 1e3 for v in t}
                kmed = {v: statistics.median(k[v]) for v in k}
                rows.append({"top": top, "hits": len(hs), "mode": name, "unit": unit,
                             "loop_ms": round(med["loop"], 3), "multi_ms": round(med["multi"], 3),
                             "loop_spread": [round(min(t["loop"]) * 1e3, 3), round(max(t["loop"]) * 1e3, 3)],
                             "multi_spread": [round(min(t["multi"]) * 1e3, 3), round(max(t["multi"]) * 1e3, 3)],
                             "loop_over_multi": round(med["loop"] / med["multi"], 2),
                             "loop_kernel_ms": round(kmed["loop"], 3), "multi_kernel_ms": round(kmed["multi"], 3),
                             "loop_kernel_spread": [round(min(k["loop"]), 3), round(max(k["loop"]), 3)],
                             "multi_kernel_spread": [round(min(k["multi"]), 3), round(max(k["multi"]), 3)],
                             "fill_ms": round(info["fill_ms"], 3), "walk_ms": round(info["walk_ms"], 3),
                             "chunks": info["chunks"], "loop_chunks": loop_chunks, "launches": info["launches"],
                             "profile_builds": info["profile_builds"], "units": info["units"], "tasks": info["tasks"],
                             "workgroups": info["workgroups"], "code_mib": round(info["code_bytes"] / 2 ** 20, 1)})

    print("unit size %d wave tasks (%s); %d queries x %d subjects; medians of %d passes taken in turn, (min ... max)"
          % (unit, a.lib or "the tree's library", a.queries, a.subjects, a.repeats))
    print(" top  hits mode    loop call ms (spread)           multi call ms (spread)        loop/multi  "
          "loop fill+walk ms (spread)      multi fill+walk ms (spread)   chunks loop/multi  launches  builds  units  code MiB")
    for r in rows:
        print(f"{r['top']:4d} {r['hits']:5d} {r['mode']:6s} "
              f"{r['loop_ms']:9.3f} ({r['loop_spread'][0]:8.3f} ... {r['loop_spread'][1]:8.3f}) "
              f"{r['multi_ms']:9.3f} ({r['multi_spread'][0]:8.3f} ... {r['multi_spread'][1]:8.3f}) {r['loop_over_multi']:10.2f} "
              f"{r['loop_kernel_ms']:9.3f} ({r['loop_kernel_spread'][0]:8.3f} ... {r['loop_kernel_spread'][1]:8.3f}) "
              f"{r['multi_kernel_ms']:9.3f} ({r['multi_kernel_spread'][0]:8.3f} ... {r['multi_kernel_spread'][1]:8.3f}) "
              f"{r['loop_chunks']:7d} / {r['chunks']:<5d} {r['launches']:9d} {r['profile_builds']:7d} {r['units']:6d} {r['code_mib']:9.1f}")
    print(json.dumps({"tool": "align_db_multi_bench", "unit": unit, "queries": a.queries, "subjects": a.subjects,
                      "tops": a.tops, "repeats": a.repeats, "results_equal": True, "rows": rows}), flush=True)


if __name__ == "__main__":
    main()
