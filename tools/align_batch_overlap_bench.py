"""What the overlap (dovetail) scores and alignments of a list of long pairs cost in one call, beside the
loop of single-pair calls.

Workload (seeded): pairs of reads that share about half their length.  Pair k is cut from one random
sequence of 1.5 x L letters (L uniform in 18-22k, shard.synthetic_batch, seeds 1000 + k): Y its first L
letters, X its last L, each mutated on its own (15 % substitutions, 2 % indels), so Y's suffix lies on X's
prefix; alphabet 20, BLOSUM62; gaps -11/-1 and -11/-11.  Everything device-resident, one process.  Per gap
model, on the first --pairs pairs: Engine.align_batch_overlap_dev (one call) beside the loop of
Engine.align_pair_overlap_dev over the same pairs, Engine.score_overlap_batch_dev beside the loop of
Engine.score_overlap_dev, and Engine.score_semi_batch_dev and Engine.score_batch_dev (the semi-global and
the global kernels, same shapes, same K) beside the batched overlap score launch; then the batch call at
scratch limits of 2, 4, 8 and 16 GiB; then the batch call alone on --many pairs.

Method: one untimed pass, then --repeats timed passes; host clock around the
synchronous calls and the hipEvent times the calls report; medians and the spread (max - min).  Every
CIGAR of both sides is replayed on the host from the call's start cell and must give the call's score and
end cell, and the two sides must agree in all six fields.  Prints a table and one JSON line and writes the
table to profiles/align_batch_overlap_ab.txt (--out)."""
import argparse
import gc
import json
import os
import re
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GAPS = [("AG", -11, -1), ("LG", -11, -11)]
FIELDS = ("score", "i_start", "j_start", "i_end", "j_end", "cigar")


def replay(cigar, y, x, i0, j0, sub, go, ge):
    """(score, i_end, j_end) of a CIGAR from (i0, j0); '=' must sit on equal letters, 'X' on different."""
    runs = [(int(c), o) for c, o in re.findall(r"(\d+)([=XID])", cigar)]
    if not runs:
        return 0, i0, j0
    cnt = np.array([c for c, _ in runs])
    ops = np.repeat(np.array([ord(o) for _, o in runs]), cnt)
    di, dj = ops != ord("D"), ops != ord("I")
    i, j = i0 + np.cumsum(di), j0 + np.cumsum(dj)
    diag = di & dj
    yy, xx = y[i[diag]], x[j[diag]]
    assert np.array_equal(yy == xx, ops[diag] == ord("="))
    score = int(sub[yy, xx].sum()) + sum(go + (c - 1) * ge for c, o in runs if o in "ID")
    return score, int(i[-1]), int(j[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=64, help="pairs of the comparison with the loop")
    ap.add_argument("--many", type=int, default=512, help="pairs of the batch-only run (0: none)")
    ap.add_argument("--limits", type=int, nargs="*", default=[2, 4, 8, 16], help="scratch limits of the sweep, GiB")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_batch_overlap_ab.txt"), help="the table's file ('' for none)")
    a = ap.parse_args()

    import torch
    import gpuseqalign_amd as gsa
    from gpuseqalign_amd import formats as F
    from gpuseqalign_amd import shard

    assert torch.cuda.is_available(), "needs cuda:0"
    dev = torch.device("cuda:0")
    sub = np.asarray(F.read_subst_json(os.path.join(ROOT, "tests", "golden", "resrc", "subst.json")).matrix("blosum62"))
    substsz = int(round(sub.size ** 0.5))
    subm = sub.reshape(substsz, substsz)
    ts = torch.from_numpy(np.ascontiguousarray(sub, dtype=np.int32).ravel().copy()).to(dev)
    up = lambda v: torch.from_numpy(np.ascontiguousarray(v, dtype=np.int32)).to(dev)

    n_all = max(a.pairs, a.many)
    host, keep, ptrs = [], [], []
    for k, (_, read) in enumerate(shard.synthetic_batch(n_all, 18000, 22000, seed0=1000)):
        L = len(read) - 1
        S = np.asarray(F.synthetic_seq(L + L // 2, 7000 + k, 20))
        Y = np.asarray(F.mutate_seq(np.concatenate([[0], S[1:1 + L]]), 5000 + k))
        X = np.asarray(F.mutate_seq(np.concatenate([[0], S[1 + L // 2:]]), 6000 + k))
        host.append((Y, X))
        ty, tx = up(Y), up(X)
        keep.append((ty, tx))
        ptrs.append((ty.data_ptr(), ty.numel(), tx.data_ptr(), tx.numel()))
    torch.cuda.synchronize(dev)

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

    def checked(res, n, go, ge):
        for k in range(n):
            r = res[k]
            assert r["status"] == 0 and (r["i_start"] == 0 or r["j_start"] == 0), (k, r["status"])
            assert replay(r["cigar"], host[k][0], host[k][1], r["i_start"], r["j_start"], subm, go, ge) == \
                (r["score"], r["i_end"], r["j_end"]), k

    t6 = lambda res: [tuple(r[f] for f in FIELDS) for r in res]
    s3 = lambda res: [(r["score"], r["i_end"], r["j_end"]) for r in res]
    rows, sweep, many = [], [], []
    with gsa.Engine(0) as eng:
        def batch(n, go, ge, limit=0):
            def run():
                r = eng.align_batch_overlap_dev(ptrs[:n], ts.data_ptr(), substsz, go, ge, 0, limit)
                run.info = eng.last_align_batch_overlap_info()
                return r, {k: run.info[k] for k in ("score_ms", "fill_ms", "walk_ms")}
            res, ms = timed(run)
            return res, ms, run.info

        for name, go, ge in GAPS:
            n = a.pairs

            def loop():
                out, acc = [], {"score_ms": 0.0, "fill_ms": 0.0, "walk_ms": 0.0}
                for p in ptrs[:n]:
                    out.append(eng.align_pair_overlap_dev(*p, ts.data_ptr(), substsz, go, ge))
                    info = eng.last_align_pair_overlap_info()
                    for k in acc:
                        acc[k] += info[k]
                return out, acc

            def score_batch():
                r = eng.score_overlap_batch_dev(ptrs[:n], ts.data_ptr(), substsz, go, ge)
                return r, {"kernel_ms": r[0]["kernel_ms"]}

            def score_semi():
                r = eng.score_semi_batch_dev(ptrs[:n], ts.data_ptr(), substsz, go, ge)
                return r, {"kernel_ms": r[0]["kernel_ms"]}

            def score_loop():
                out = [eng.score_overlap_dev(*p, ts.data_ptr(), substsz, go, ge) for p in ptrs[:n]]
                return out, {"kernel_ms": sum(r["kernel_ms"] for r in out)}

            def score_global():
                r = eng.score_batch_dev(ptrs[:n], ts.data_ptr(), substsz, go, ge, False)
                return r, {"kernel_ms": r[0]["kernel_ms"]}

            bres, bms, info = batch(n, go, ge)
            lres, lms = timed(loop)
            sb, sbms = timed(score_batch)
            sl, slms = timed(score_loop)
            _, sgms = timed(score_global)
            _, ssms = timed(score_semi)
            checked(bres, n, go, ge)
            checked(lres, n, go, ge)
            assert t6(bres) == t6(lres) and s3(sb) == s3(sl) == s3(bres)
            assert info["batch_pairs"] == n, info
            row = {"gaps": name, "pairs": n, "strips": info["strips"], "rounds": info["rounds"],
                   "code_gib": round(info["code_bytes"] / 2 ** 30, 2), "gran_gib": round(info["gran_bytes"] / 2 ** 30, 2),
                   "strips_filled": info["strips_filled"],
                   "overlap_over_semi_kernel": round(sbms["kernel_ms"][0] / ssms["kernel_ms"][0], 3),
                   "loop_over_batch": round(lms["call_ms"][0] / bms["call_ms"][0], 2),
                   "score_loop_over_batch": round(slms["call_ms"][0] / sbms["call_ms"][0], 2),
                   "overlap_over_global_kernel": round(sbms["kernel_ms"][0] / sgms["kernel_ms"][0], 3)}
            for side, ms in (("batch", bms), ("loop", lms), ("sbatch", sbms), ("sloop", slms), ("sglobal", sgms), ("ssemi", ssms)):
                for k, v in ms.items():
                    row[side + "_" + k], row[side + "_" + k + "_spread"] = round(v[0], 2), round(v[1], 2)
            rows.append(row)
            print(name, "batch and loop done", file=sys.stderr, flush=True)
            for gib in a.limits:
                res, ms, inf = batch(n, go, ge, gib << 30)
                assert t6(res) == t6(bres)
                sweep.append({"gaps": name, "pairs": n, "limit_gib": gib, "rounds": inf["rounds"], "strips": inf["strips"],
                              "strips_filled": inf["strips_filled"], "code_gib": round(inf["code_bytes"] / 2 ** 30, 2),
                              **{k: round(v[0], 2) for k, v in ms.items()}, "call_ms_spread": round(ms["call_ms"][1], 2)})
            if a.many:
                res, ms, inf = batch(a.many, go, ge)
                checked(res, a.many, go, ge)
                assert inf["batch_pairs"] == a.many, inf
                many.append({"gaps": name, "pairs": a.many, "strips": inf["strips"], "strips_filled": inf["strips_filled"],
                             "rounds": inf["rounds"], "code_gib": round(inf["code_bytes"] / 2 ** 30, 2),
                             **{k: round(v[0], 2) for k, v in ms.items()}, "call_ms_spread": round(ms["call_ms"][1], 2)})
                print(name, "many done", file=sys.stderr, flush=True)

    lines = []
    lines.append("pairs of reads of 18-22k that share about half their length, each mutated on its own (15 %% substitutions, 2 %% "
                 "indels), BLOSUM62, device-resident; one untimed pass, then %d timed: medians (spread = max - min)" % a.repeats)
    lines.append("batch = one Engine.align_batch_overlap_dev call; loop = Engine.align_pair_overlap_dev pair by pair; sum = score + fill "
                 "+ walk (hipEvent); every CIGAR of both sides replayed on the host, both sides equal in all six fields")
    lines.append("gaps pairs strips filled rounds codes GiB rows GiB | batch call ms (spread)   score    fill    walk     sum | loop call ms "
                 "(spread)   score     fill     walk      sum | loop/batch")
    for r in rows:
        bs = r["batch_score_ms"] + r["batch_fill_ms"] + r["batch_walk_ms"]
        ls = r["loop_score_ms"] + r["loop_fill_ms"] + r["loop_walk_ms"]
        lines.append(f"{r['gaps']:4s} {r['pairs']:5d} {r['strips']:6d} {r['strips_filled']:6d} {r['rounds']:6d} {r['code_gib']:9.2f} {r['gran_gib']:8.2f} | "
                     f"{r['batch_call_ms']:13.2f} ({r['batch_call_ms_spread']:6.2f}) {r['batch_score_ms']:7.2f} {r['batch_fill_ms']:7.2f} "
                     f"{r['batch_walk_ms']:7.2f} {bs:7.2f} | {r['loop_call_ms']:12.2f} ({r['loop_call_ms_spread']:6.2f}) "
                     f"{r['loop_score_ms']:8.2f} {r['loop_fill_ms']:8.2f} {r['loop_walk_ms']:8.2f} {ls:8.2f} | {r['loop_over_batch']:10.2f}")
    lines.append("")
    lines.append("scores alone: Engine.score_overlap_batch_dev beside the loop of Engine.score_overlap_dev, and beside "
                 "Engine.score_semi_batch_dev and Engine.score_batch_dev (semi-global and global, same shapes and K):")
    lines.append("gaps pairs | batch call ms (spread) kernel ms | loop call ms (spread) kernel ms | loop/batch | global batch kernel ms "
                 "(spread) | overlap/global kernel | semi batch kernel ms (spread) | overlap/semi kernel")
    for r in rows:
        lines.append(f"{r['gaps']:4s} {r['pairs']:5d} | {r['sbatch_call_ms']:13.2f} ({r['sbatch_call_ms_spread']:6.2f}) "
                     f"{r['sbatch_kernel_ms']:9.2f} | {r['sloop_call_ms']:12.2f} ({r['sloop_call_ms_spread']:6.2f}) "
                     f"{r['sloop_kernel_ms']:9.2f} | {r['score_loop_over_batch']:10.2f} | {r['sglobal_kernel_ms']:22.2f} "
                     f"({r['sglobal_kernel_ms_spread']:6.2f}) | {r['overlap_over_global_kernel']:21.3f} | {r['ssemi_kernel_ms']:20.2f} "
                     f"({r['ssemi_kernel_ms_spread']:6.2f}) | {r['overlap_over_semi_kernel']:19.3f}")
    for title, tab in (("the batch call at other scratch limits:", sweep), ("the batch call alone on more pairs:", many)):
        if not tab:
            continue
        lines.append("")
        lines.append(title)
        lines.append("gaps pairs limit GiB strips filled rounds codes GiB | call ms (spread)   score    fill    walk")
        for r in tab:
            lim = "%9d" % r["limit_gib"] if "limit_gib" in r else "  default"
            lines.append(f"{r['gaps']:4s} {r['pairs']:5d} {lim} {r['strips']:6d} {r['strips_filled']:6d} {r['rounds']:6d} {r['code_gib']:9.2f} | {r['call_ms']:8.2f} "
                         f"({r['call_ms_spread']:6.2f}) {r['score_ms']:7.2f} {r['fill_ms']:7.2f} {r['walk_ms']:7.2f}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps({"tool": "align_batch_overlap_bench", "repeats": a.repeats, "rows": rows, "sweep": sweep, "many": many}), flush=True)


if __name__ == "__main__":
    main()
