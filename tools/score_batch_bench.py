"""Batched score-only alignment against a loop of single-pair calls.

64 and 512 synthetic pairs of 18-22k (shard.synthetic_batch, the BASELINE configs[3] generator),
NW-LG, SW-LG and NW-AG, device-resident: one Engine.score_batch_dev call against a loop of
Engine.score_dev over the same pairs, in the same process.  The loop is the library's single-pair
path with its own choices (rows per lane, both ends); the batch runs with its defaults, with
GSA_SCORE_K forced to 2, and at 4 rows per lane with the int8 and the int16 column profile
(GSA_KROW_Q8 = 2 / 0).  Per variant: one untimed pass, then --repeats timed
passes taken in turn (batch variants and loop alternate), host clock around the synchronous calls;
the median is reported, with the passes' spread.  Every batch result must equal the loop's.
Prints a table and one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODES = [("NW-LG", -11, -11, False), ("SW-LG", -11, -11, True), ("NW-AG", -11, -1, False)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, nargs="+", default=[64, 512])
    ap.add_argument("--lo", type=int, default=18000)
    ap.add_argument("--hi", type=int, default=22000)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()

    import torch
    import gpuseqalign_amd as gsa
    from gpuseqalign_amd import shard, formats as F

    assert torch.cuda.is_available(), "needs cuda:0"
    dev = torch.device("cuda:0")
    sub = F.read_subst_json(os.path.join(ROOT, "tests", "golden", "resrc", "subst.json")).matrix("blosum62")
    substsz = int(round(sub.size ** 0.5))
    ts = torch.from_numpy(sub.ravel().copy()).to(dev)
    rows = []
    with gsa.Engine(0) as eng:
        for n in a.pairs:
            pairs = shard.synthetic_batch(n, a.lo, a.hi, seed0=1000)
            ins = [(torch.from_numpy(y).to(dev), torch.from_numpy(x).to(dev)) for y, x in pairs]
            ptrs = [(y.data_ptr(), len(y), x.data_ptr(), len(x)) for y, x in ins]
            cells = sum((len(y) - 1) * (len(x) - 1) for y, x in pairs)
            torch.cuda.synchronize(dev)
            for name, go, ge, local in MODES:
                def batch(k, q8=None):
                    eng.set_knob("GSA_SCORE_K", k)
                    eng.set_knob("GSA_KROW_Q8", q8)
                    t0 = time.perf_counter()
                    r = eng.score_batch_dev(ptrs, ts.data_ptr(), substsz, go, ge, local)
                    dt = time.perf_counter() - t0
                    ll = eng.last_launch()
                    assert ll["kind"] == "score_krow" and ll["npairs"] == n, ll
                    eng.set_knob("GSA_SCORE_K", None)
                    eng.set_knob("GSA_KROW_Q8", None)
                    return dt, [(d["score"], d["i_end"], d["j_end"]) for d in r], ll["k"]

                def loop():
                    t0 = time.perf_counter()
                    r = [eng.score_dev(*p, ts.data_ptr(), substsz, go, ge, local) for p in ptrs]
                    dt = time.perf_counter() - t0
                    return dt, [(d["score"], d["i_end"], d["j_end"]) for d in r], eng.last_launch()["k"]

                variants = [("batch", lambda: batch(None)), ("batch K=2", lambda: batch("2")),
                            ("batch K=4 i8", lambda: batch("4", "2")), ("batch K=4 i16", lambda: batch("4", "0")),
                            ("loop", loop)]
                times = {v: [] for v, _ in variants}
                got, ks = {}, {}
                for it in range(1 + a.repeats):  # pass 0: warm-up
                    for v, fn in variants:
                        dt, got[v], ks[v] = fn()
                        if it:
                            times[v].append(dt)
                for v, _ in variants:
                    assert got[v] == got["loop"], (n, name, v)
                med = {v: statistics.median(t) for v, t in times.items()}
                for v, _ in variants:
                    rows.append({"pairs": n, "mode": name, "variant": v, "k": ks[v], "ms": round(med[v] * 1e3, 2),
                                 "min_ms": round(min(times[v]) * 1e3, 2), "max_ms": round(max(times[v]) * 1e3, 2),
                                 "gcups": round(cells / med[v] / 1e9, 1),
                                 "vs_loop": round(med["loop"] / med[v], 2)})
    print("pairs mode   variant        K      ms (min .. max)            GCUPS  loop/this")
    for r in rows:
        print(f"{r['pairs']:5d} {r['mode']:6s} {r['variant']:13s} {r['k']:2d} {r['ms']:9.2f} ({r['min_ms']:.2f} .. "
              f"{r['max_ms']:.2f}) {r['gcups']:9.1f} {r['vs_loop']:7.2f}")
    print(json.dumps({"tool": "score_batch_bench", "lengths": [a.lo, a.hi], "repeats": a.repeats,
                      "results_equal": True, "rows": rows}), flush=True)


if __name__ == "__main__":
    main()
