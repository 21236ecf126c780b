"""What the banded calls cost over a list of related long pairs in one call, beside the loop of single-pair
banded calls and beside the unbanded batch calls.

Workload (seeded): the pairs of tools/align_batch_bench.py (shard.synthetic_batch: lengths uniform in
18-22k, seeds 1000 + k; seqX the generator's, seqY a mutated copy of it: 15 % substitutions, 2 % indels);
alphabet 20, BLOSUM62, NW-AG -11 / -1; --pairs pairs (64 and 512) and --bands diagonals (512 and 2048) on
either side of the ones (0, 0) and (R, C) need.  Everything device-resident.

Per pair count and band, one step: Engine.align_batch_band_dev and Engine.score_band_batch_dev with
waves = 0 and with waves = 16 forced, beside
  the loop of Engine.align_pair_band_dev / Engine.score_band_dev over the same pairs (up to --loop-max pairs),
  Engine.align_batch_dev / Engine.score_batch_dev (unbanded) on the same pairs,
all in the same process and run.  The yardsticks are the other calls, never the new call against itself.

Method: one untimed pass, then --repeats timed passes; host clock around the synchronous
calls and the hipEvent times the calls report; medians and the spread (max - min).  Every CIGAR of the
batched call is replayed on the host and must give the call's score, and the batched call must agree with
the loop in all six fields.  Every step runs in a child process of its own under its own time limit, and
the tool stops at the first step that fails.  Prints a table and one JSON line and writes the table to
profiles/align_batch_band_ab.txt (--out)."""
import argparse
import gc
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FIELDS = ("score", "i_start", "j_start", "i_end", "j_end", "cigar")
GO, GE = -11, -1


def step(n, band, repeats, loop_max):
    import torch
    import gpuseqalign_amd as gsa
    from gpuseqalign_amd import formats as F
    from gpuseqalign_amd import shard
    from tests import _align_oracle as ao

    assert torch.cuda.is_available(), "needs cuda:0"
    dev = torch.device("cuda:0")
    sub = np.asarray(F.read_subst_json(os.path.join(ROOT, "tests", "golden", "resrc", "subst.json")).matrix("blosum62"))
    substsz = int(round(sub.size ** 0.5))
    subm = sub.reshape(substsz, substsz)
    ts = torch.from_numpy(np.ascontiguousarray(sub, dtype=np.int32).ravel().copy()).to(dev)
    host, keep, ptrs, bands = [], [], [], []
    for k, (_, X) in enumerate(shard.synthetic_batch(n, 18000, 22000, seed0=1000)):
        Y = F.mutate_seq(X, 5000 + k)
        host.append((np.asarray(Y), np.asarray(X)))
        ty = torch.from_numpy(np.ascontiguousarray(Y, dtype=np.int32)).to(dev)
        tx = torch.from_numpy(np.ascontiguousarray(X, dtype=np.int32)).to(dev)
        keep.append((ty, tx))
        ptrs.append((ty.data_ptr(), ty.numel(), tx.data_ptr(), tx.numel()))
        R, C = len(Y) - 1, len(X) - 1
        bands.append((min(0, C - R) - band, max(0, C - R) + band))
    torch.cuda.synchronize(dev)

    def timed(fn):
        """fn -> (value, {name: (median ms, spread ms)}); one untimed pass, then the timed ones."""
        acc, val = {}, None
        for it in range(1 + repeats):
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
        return val, {k: (round(statistics.median(v), 3), round(max(v) - min(v), 3)) for k, v in acc.items()}

    row = {"pairs": n, "band": band}
    with gsa.Engine(0) as eng:
        tp = ts.data_ptr()

        def balign(waves):
            def run():
                r = eng.align_batch_band_dev(ptrs, tp, substsz, GO, GE, bands=bands, waves=waves)
                info = eng.last_align_batch_band_info()
                run.info = info
                return r, {k: info[k] for k in ("fill_ms", "walk_ms", "nocode_ms")}
            return run

        def bscore(waves):
            def run():
                r = eng.score_band_batch_dev(ptrs, tp, substsz, GO, GE, bands=bands, waves=waves)
                return r, {"kernel_ms": r[0]["kernel_ms"]}
            return run

        def loop_align():
            out = [eng.align_pair_band_dev(*p, tp, substsz, GO, GE, lo, hi, 8 << 30) for p, (lo, hi) in zip(ptrs, bands)]
            return out, {}

        def loop_score():
            out = [eng.score_band_dev(*p, tp, substsz, GO, GE, lo, hi) for p, (lo, hi) in zip(ptrs, bands)]
            return out, {"kernel_ms": sum(r["kernel_ms"] for r in out)}

        def full_align():
            r = eng.align_batch_dev(ptrs, tp, substsz, GO, GE)
            info = eng.last_align_batch_info()
            return r, {k: info[k] for k in ("score_ms", "fill_ms", "walk_ms")}

        def full_score():
            r = eng.score_batch_dev(ptrs, tp, substsz, GO, GE)
            return r, {"kernel_ms": r[0]["kernel_ms"]}

        run0 = balign(0)
        b0, row["batch_align"] = timed(run0)
        info = run0.info
        b16, row["batch_align_w16"] = timed(balign(16))
        s0, row["batch_score"] = timed(bscore(0))
        s16, row["batch_score_w16"] = timed(bscore(16))
        row.update(waves=info["waves"], rounds=info["rounds"], code_gib=round(info["code_bytes"] / 2 ** 30, 3),
                   nocode_pairs=info["nocode_pairs"], proved=sum(q["proved_optimal"] for q in info["pairs"]),
                   supersteps_max=max(q["supersteps"] for q in info["pairs"]),
                   supersteps_sum=sum(q["supersteps"] for q in info["pairs"]))
        strip = lambda rs: [{k: r[k] for k in FIELDS + ("status",)} for r in rs]
        assert strip(b0) == strip(b16) and [r["score"] for r in s0] == [r["score"] for r in s16] == [r["score"] for r in b0]
        for k, r in enumerate(b0):
            assert r["status"] == 0, (k, r["status"])
            assert ao.rescore(r["cigar"], host[k][0], host[k][1], 0, 0, subm, GO, GE) == (r["score"], r["i_end"], r["j_end"]), k
        if n <= loop_max:
            la, row["loop_align"] = timed(loop_align)
            ls, row["loop_score"] = timed(loop_score)
            assert strip(la) == strip(b0) and [r["score"] for r in ls] == [r["score"] for r in s0]
        fa, row["full_align"] = timed(full_align)
        fs, row["full_score"] = timed(full_score)
        row["same_score_as_unbanded"] = sum(int(a["score"] == b["score"]) for a, b in zip(b0, fs))
        row["same_cigar_as_unbanded"] = sum(int(a["cigar"] == b["cigar"]) for a, b in zip(b0, fa))
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, nargs="*", default=[64, 512])
    ap.add_argument("--bands", type=int, nargs="*", default=[512, 2048])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--loop-max", type=int, default=64, help="most pairs the loop of single-pair calls is run on")
    ap.add_argument("--step-timeout", type=int, default=420, help="seconds a step may take")
    ap.add_argument("--step", type=int, nargs=2, default=None, help="(internal) run one step: pairs band")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_batch_band_ab.txt"), help="the table's file ('' for none)")
    a = ap.parse_args()
    if a.step:
        step(a.step[0], a.step[1], a.repeats, a.loop_max)
        return

    rows = []
    for n in a.pairs:
        for band in a.bands:
            cmd = [sys.executable, os.path.abspath(__file__), "--step", str(n), str(band), "--repeats", str(a.repeats),
                   "--loop-max", str(a.loop_max)]
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.step_timeout)
            if p.returncode != 0:
                sys.stderr.write(p.stdout + p.stderr)
                sys.exit("step %d pairs, band %d failed with status %d: stopping" % (n, band, p.returncode))
            rows.append(json.loads(p.stdout.strip().split("\n")[-1]))
            print("step %d pairs, band %d: done" % (n, band), file=sys.stderr, flush=True)

    def ms(r, key, name="call_ms"):
        return "%9.3f (%7.3f)" % tuple(r[key][name]) if key in r else "          not run"

    lines = []
    lines.append("related pairs of 18-22k letters (15 %% substitutions, 2 %% indels), BLOSUM62 -11 / -1, device-resident; per "
                 "row one process; one untimed pass, then %d timed: medians (spread = max - min), ms" % a.repeats)
    lines.append("batch = Engine.align_batch_band_dev / Engine.score_band_batch_dev, waves = 0 and waves = 16 forced; loop = "
                 "Engine.align_pair_band_dev / Engine.score_band_dev over the same pairs; unbanded = Engine.align_batch_dev / "
                 "Engine.score_batch_dev on the same pairs; call: host clock around the synchronous call(s), the others "
                 "hipEvent times; every batched CIGAR replayed, batch == loop in all six fields")
    for r in rows:
        lines.append("pairs %d band %d: waves %d rounds %d codes %.3f GiB proved %d / %d  super-steps max %d sum %d  "
                     "=score as unbanded %d =cigar %d" % (r["pairs"], r["band"], r["waves"], r["rounds"], r["code_gib"], r["proved"],
                                                          r["pairs"], r["supersteps_max"], r["supersteps_sum"],
                                                          r["same_score_as_unbanded"], r["same_cigar_as_unbanded"]))
        lines.append("  align  batch call %s = fill %s + walk %s | waves 16 call %s fill %s" % (
            ms(r, "batch_align"), ms(r, "batch_align", "fill_ms"), ms(r, "batch_align", "walk_ms"), ms(r, "batch_align_w16"),
            ms(r, "batch_align_w16", "fill_ms")))
        lines.append("         loop  call %s | unbanded call %s = score %s + fill %s + walk %s" % (
            ms(r, "loop_align"), ms(r, "full_align"), ms(r, "full_align", "score_ms"), ms(r, "full_align", "fill_ms"),
            ms(r, "full_align", "walk_ms")))
        lines.append("  score  batch call %s kernel %s | waves 16 call %s kernel %s" % (
            ms(r, "batch_score"), ms(r, "batch_score", "kernel_ms"), ms(r, "batch_score_w16"), ms(r, "batch_score_w16", "kernel_ms")))
        lines.append("         loop  call %s kernel %s | unbanded call %s kernel %s" % (
            ms(r, "loop_score"), ms(r, "loop_score", "kernel_ms"), ms(r, "full_score"), ms(r, "full_score", "kernel_ms")))
        lines.append("  waves 16 / waves 0: align fill %.2f x, score kernel %.2f x" % (
            r["batch_align_w16"]["fill_ms"][0] / r["batch_align"]["fill_ms"][0],
            r["batch_score_w16"]["kernel_ms"][0] / r["batch_score"]["kernel_ms"][0]))
        if "loop_align" in r:
            lines.append("  loop / batch: align call %.1f x, score call %.1f x" % (
                r["loop_align"]["call_ms"][0] / r["batch_align"]["call_ms"][0],
                r["loop_score"]["call_ms"][0] / r["batch_score"]["call_ms"][0]))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps({"tool": "align_batch_band_bench", "pairs": a.pairs, "bands": a.bands, "repeats": a.repeats, "rows": rows}),
          flush=True)


if __name__ == "__main__":
    main()
