"""What the banded extension calls cost, in four parts, all in one run on one box:

  a  the running maximum: the fill kernels of Engine.align_batch_band_ext_dev / score_band_ext_batch_dev beside
     those of Engine.align_batch_band_dev / score_band_batch_dev on the same related pairs of 18-22k letters
     (tools/align_batch_band_bench.py's: 15 % substitutions, 2 % indels) with 512 diagonals on either side of
     the ones (0, 0) and (R, C) need -- a band both modes take, so both fill the same cells -- for 64 and 512
     pairs and the affine (-11 / -1) and the linear (-4 / -4) gap model;
  b  the extension batch beside the loop of Engine.align_pair_band_ext_dev / score_band_ext_dev over the same
     64 pairs;
  c  read ends: 512 pairs of 2-10k letters, related for their first 30-90 % and unrelated behind, band=128: the
     call and its split, the same pairs through Engine.align_batch_band_dev (128 diagonals beyond the ones the
     corner needs: what a caller paid before), and how far the extensions ran;
  d  trimming: 64 queries of 20k letters against subjects of 5k, band=128: the super-steps the call ran beside
     the untrimmed plan's count, and its time.

Method: one untimed pass, then --repeats timed passes; host clock around the synchronous calls
and the hipEvent times the calls report; medians and the spread (max - min).  Every CIGAR of the extension
batch is replayed on the host and must give the call's score and end cell; in b the batch must agree with the
loop in all six fields.  Every step runs in a child process of its own under its own time limit, and the tool
stops at the first step that fails.  Prints a table and one JSON line and writes the table to
profiles/align_batch_band_ext_ab.txt (--out)."""
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
TR, LAG = 256, 6


def _setup():
    import torch
    from gpuseqalign_amd import formats as F
    assert torch.cuda.is_available(), "needs cuda:0"
    dev = torch.device("cuda:0")
    sub = np.asarray(F.read_subst_json(os.path.join(ROOT, "tests", "golden", "resrc", "subst.json")).matrix("blosum62"))
    substsz = int(round(sub.size ** 0.5))
    ts = torch.from_numpy(np.ascontiguousarray(sub, dtype=np.int32).ravel().copy()).to(dev)
    return torch, dev, sub.reshape(substsz, substsz), substsz, ts


def _upload(torch, dev, host):
    keep, ptrs = [], []
    for Y, X in host:
        ty = torch.from_numpy(np.ascontiguousarray(Y, dtype=np.int32)).to(dev)
        tx = torch.from_numpy(np.ascontiguousarray(X, dtype=np.int32)).to(dev)
        keep.append((ty, tx))
        ptrs.append((ty.data_ptr(), ty.numel(), tx.data_ptr(), tx.numel()))
    torch.cuda.synchronize(dev)
    return keep, ptrs


def _timed(fn, repeats):
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


def _calls(eng, ptrs, tp, substsz, go, ge):
    def ext_align(bands):
        def run():
            r = eng.align_batch_band_ext_dev(ptrs, tp, substsz, go, ge, bands=bands)
            run.info = eng.last_align_batch_band_ext_info()
            return r, {k: run.info[k] for k in ("fill_ms", "walk_ms", "nocode_ms")}
        return run

    def ext_score(bands):
        def run():
            r = eng.score_band_ext_batch_dev(ptrs, tp, substsz, go, ge, bands=bands)
            return r, {"kernel_ms": r[0]["kernel_ms"]}
        return run

    def glob_align(bands):
        def run():
            r = eng.align_batch_band_dev(ptrs, tp, substsz, go, ge, bands=bands)
            run.info = eng.last_align_batch_band_info()
            return r, {k: run.info[k] for k in ("fill_ms", "walk_ms", "nocode_ms")}
        return run

    def glob_score(bands):
        def run():
            r = eng.score_band_batch_dev(ptrs, tp, substsz, go, ge, bands=bands)
            return r, {"kernel_ms": r[0]["kernel_ms"]}
        return run

    return ext_align, ext_score, glob_align, glob_score


def _replay(results, host, subm, go, ge):
    from tests import _align_oracle as ao
    for k, r in enumerate(results):
        assert r["status"] == 0, (k, r["status"])
        assert ao.rescore(r["cigar"], host[k][0], host[k][1], 0, 0, subm, go, ge) == (r["score"], r["i_end"], r["j_end"]), k


def _long_pairs(n):
    from gpuseqalign_amd import formats as F
    from gpuseqalign_amd import shard
    host = []
    for k, (_, X) in enumerate(shard.synthetic_batch(n, 18000, 22000, seed0=1000)):
        host.append((np.asarray(F.mutate_seq(X, 5000 + k)), np.asarray(X)))
    return host


def step_a(n, go, ge, repeats):
    import gpuseqalign_amd as gsa
    torch, dev, subm, substsz, ts = _setup()
    host = _long_pairs(n)
    keep, ptrs = _upload(torch, dev, host)
    bands = [(min(0, len(X) - len(Y)) - 512, max(0, len(X) - len(Y)) + 512) for Y, X in host]
    row = {"part": "a", "pairs": n, "go": go, "ge": ge}
    with gsa.Engine(0) as eng:
        ea, es, ga, gs = _calls(eng, ptrs, ts.data_ptr(), substsz, go, ge)
        run = ea(bands)
        e, row["ext_align"] = _timed(run, repeats)
        _replay(e, host, subm, go, ge)
        row["corner"] = sum(int((r["i_end"], r["j_end"]) == (len(Y) - 1, len(X) - 1)) for r, (Y, X) in zip(e, host))
        row["rows_used"], row["cols_used"] = run.info["rows_used"], run.info["cols_used"]
        row["rows"], row["cols"] = sum(len(Y) - 1 for Y, _ in host), sum(len(X) - 1 for _, X in host)
        g, row["glob_align"] = _timed(ga(bands), repeats)
        s, row["ext_score"] = _timed(es(bands), repeats)
        t, row["glob_score"] = _timed(gs(bands), repeats)
        assert [r["score"] for r in s] == [r["score"] for r in e] and [r["score"] for r in t] == [r["score"] for r in g]
        assert all(a["score"] >= b["score"] for a, b in zip(e, g))  # the corner is one of the cells
    print(json.dumps(row), flush=True)


def step_b(n, go, ge, repeats):
    import gpuseqalign_amd as gsa
    torch, dev, subm, substsz, ts = _setup()
    host = _long_pairs(n)
    keep, ptrs = _upload(torch, dev, host)
    bands = [(-512, 512)] * n
    row = {"part": "b", "pairs": n, "go": go, "ge": ge}
    with gsa.Engine(0) as eng:
        tp = ts.data_ptr()
        ea, es, _, _ = _calls(eng, ptrs, tp, substsz, go, ge)
        e, row["ext_align"] = _timed(ea(bands), repeats)
        s, row["ext_score"] = _timed(es(bands), repeats)

        def loop_align():
            return [eng.align_pair_band_ext_dev(*p, tp, substsz, go, ge, -512, 512, 8 << 30) for p in ptrs], {}

        def loop_score():
            out = [eng.score_band_ext_dev(*p, tp, substsz, go, ge, -512, 512) for p in ptrs]
            return out, {"kernel_ms": sum(r["kernel_ms"] for r in out)}

        la, row["loop_align"] = _timed(loop_align, repeats)
        ls, row["loop_score"] = _timed(loop_score, repeats)
        strip = lambda rs: [{k: r[k] for k in FIELDS + ("status",)} for r in rs]
        assert strip(la) == strip(e) and [(r["score"], r["i_end"], r["j_end"]) for r in ls] == [(r["score"], r["i_end"], r["j_end"]) for r in s]
    print(json.dumps(row), flush=True)


def step_c(n, go, ge, repeats):
    import gpuseqalign_amd as gsa
    from gpuseqalign_amd import formats as F
    from gpuseqalign_amd import shard
    torch, dev, subm, substsz, ts = _setup()
    rng = np.random.default_rng(7)
    host, fracs = [], []
    for k, (_, X) in enumerate(shard.synthetic_batch(n, 2000, 10000, seed0=3000)):
        X = np.asarray(X)
        Y = np.asarray(F.mutate_seq(X, 7000 + k)).copy()
        f = float(rng.uniform(0.3, 0.9))
        cut = 1 + int(f * (len(Y) - 1))
        Y[cut:] = rng.integers(int(X[1:].min()), int(X[1:].max()) + 1, size=len(Y) - cut)  # unrelated behind the cut
        host.append((Y, X))
        fracs.append(f)
    keep, ptrs = _upload(torch, dev, host)
    row = {"part": "c", "pairs": n, "go": go, "ge": ge}
    with gsa.Engine(0) as eng:
        ea, es, ga, gs = _calls(eng, ptrs, ts.data_ptr(), substsz, go, ge)
        run = ea([(-128, 128)] * n)
        e, row["ext_align"] = _timed(run, repeats)
        _replay(e, host, subm, go, ge)
        s, row["ext_score"] = _timed(es([(-128, 128)] * n), repeats)
        gb = [(min(0, len(X) - len(Y)) - 128, max(0, len(X) - len(Y)) + 128) for Y, X in host]
        g, row["glob_align"] = _timed(ga(gb), repeats)
        reach = [r["i_end"] / (len(Y) - 1) for r, (Y, _) in zip(e, host)]
        row["reach_over_related"] = round(statistics.median(a / f for a, f in zip(reach, fracs)), 3)
        row["proved"] = sum(q["proved_optimal"] for q in run.info["pairs"])
        row["cigar_letters_ext"] = sum(r["i_end"] + r["j_end"] for r in e)
        row["cigar_letters_glob"] = sum(r["i_end"] + r["j_end"] for r in g)
    print(json.dumps(row), flush=True)


def step_d(n, go, ge, repeats):
    import gpuseqalign_amd as gsa
    from gpuseqalign_amd import formats as F
    from gpuseqalign_amd import shard
    torch, dev, subm, substsz, ts = _setup()
    host = []
    for k, (_, Q) in enumerate(shard.synthetic_batch(n, 20000, 20000, seed0=4000)):
        Q = np.asarray(Q)
        X = np.asarray(F.mutate_seq(Q[:5001], 9000 + k))  # a subject related to the query's first 5k letters
        host.append((Q, X))
    keep, ptrs = _upload(torch, dev, host)
    row = {"part": "d", "pairs": n, "go": go, "ge": ge}
    with gsa.Engine(0) as eng:
        ea, es, _, _ = _calls(eng, ptrs, ts.data_ptr(), substsz, go, ge)
        run = ea([(-128, 128)] * n)
        e, row["ext_align"] = _timed(run, repeats)
        _replay(e, host, subm, go, ge)
        s, row["ext_score"] = _timed(es([(-128, 128)] * n), repeats)
        q = run.info["pairs"]
        nq = -(-(257 + TR - 1 + 63) // 64)
        row["supersteps"] = sum(p["supersteps"] for p in q)
        row["supersteps_untrimmed"] = sum((-(-(len(Y) - 1) // TR) - 1) * LAG + nq for Y, _ in host)
        row["rows_used"], row["rows"] = sum(p["rows_used"] for p in q), sum(len(Y) - 1 for Y, _ in host)
    print(json.dumps(row), flush=True)


STEPS = {"a": step_a, "b": step_b, "c": step_c, "d": step_d}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", nargs="*", default=["a", "b", "c", "d"])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--step-timeout", type=int, default=300, help="seconds a step may take")
    ap.add_argument("--step", nargs=4, default=None, help="(internal) run one step: part pairs go ge")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_batch_band_ext_ab.txt"), help="the table's file ('' for none)")
    a = ap.parse_args()
    if a.step:
        STEPS[a.step[0]](int(a.step[1]), int(a.step[2]), int(a.step[3]), a.repeats)
        return

    plan = {"a": [(n, go, ge) for go, ge in ((-11, -1), (-4, -4)) for n in (64, 512)], "b": [(64, -11, -1)],
            "c": [(512, -11, -1)], "d": [(64, -11, -1)]}
    rows = []
    for part in a.parts:
        for n, go, ge in plan[part]:
            cmd = [sys.executable, os.path.abspath(__file__), "--step", part, str(n), str(go), str(ge), "--repeats", str(a.repeats)]
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.step_timeout)
            if p.returncode != 0:
                sys.stderr.write(p.stdout + p.stderr)
                sys.exit("step %s, %d pairs, %d / %d failed with status %d: stopping" % (part, n, go, ge, p.returncode))
            rows.append(json.loads(p.stdout.strip().split("\n")[-1]))
            print("step %s, %d pairs, %d / %d: done" % (part, n, go, ge), file=sys.stderr, flush=True)

    def ms(r, key, name="call_ms"):
        return "%9.3f (%7.3f)" % tuple(r[key][name]) if key in r else "          not run"

    def ratio(r, a, b, name):
        return r[a][name][0] / r[b][name][0]

    lines = ["BLOSUM62, device-resident; per row one process; one untimed pass, then %d timed: medians (spread = max - min), "
             "ms; call: host clock around the synchronous call(s), the others hipEvent times; every CIGAR of the extension "
             "batch replayed to its score and end cell" % a.repeats]
    for r in rows:
        head = "%s  pairs %d gaps %d / %d" % (r["part"], r["pairs"], r["go"], r["ge"])
        if r["part"] == "a":
            lines.append("%s: related pairs of 18-22k, 512 diagonals on either side; the extension ends in the corner for %d; "
                         "rows used %d of %d" % (head, r["corner"], r["rows_used"], r["rows"]))
            lines.append("  fill with codes   extension %s  global %s  ratio %.3f" % (
                ms(r, "ext_align", "fill_ms"), ms(r, "glob_align", "fill_ms"), ratio(r, "ext_align", "glob_align", "fill_ms")))
            lines.append("  fill without      extension %s  global %s  ratio %.3f" % (
                ms(r, "ext_score", "kernel_ms"), ms(r, "glob_score", "kernel_ms"), ratio(r, "ext_score", "glob_score", "kernel_ms")))
            lines.append("  align call        extension %s  global %s | walk extension %s global %s" % (
                ms(r, "ext_align"), ms(r, "glob_align"), ms(r, "ext_align", "walk_ms"), ms(r, "glob_align", "walk_ms")))
        elif r["part"] == "b":
            lines.append("%s: the same pairs, band (-512, 512), batch beside the loop of single calls (equal in all six fields)" % head)
            lines.append("  align  batch call %s  loop call %s  loop / batch %.1f x" % (
                ms(r, "ext_align"), ms(r, "loop_align"), ratio(r, "loop_align", "ext_align", "call_ms")))
            lines.append("  score  batch call %s  loop call %s  loop / batch %.1f x" % (
                ms(r, "ext_score"), ms(r, "loop_score"), ratio(r, "loop_score", "ext_score", "call_ms")))
        elif r["part"] == "c":
            lines.append("%s: read ends of 2-10k, related for the first 30-90 %%, band=128; median reach / related part %.3f; "
                         "proved %d; CIGAR letters extension %d, global %d" % (
                             head, r["reach_over_related"], r["proved"], r["cigar_letters_ext"], r["cigar_letters_glob"]))
            lines.append("  extension align call %s = fill %s + walk %s | score call %s kernel %s" % (
                ms(r, "ext_align"), ms(r, "ext_align", "fill_ms"), ms(r, "ext_align", "walk_ms"), ms(r, "ext_score"),
                ms(r, "ext_score", "kernel_ms")))
            lines.append("  global    align call %s = fill %s + walk %s (band: 128 beyond the corner's diagonals)" % (
                ms(r, "glob_align"), ms(r, "glob_align", "fill_ms"), ms(r, "glob_align", "walk_ms")))
        else:
            lines.append("%s: queries of 20k against subjects of 5k, band=128: super-steps %d (untrimmed plan %d), rows used %d "
                         "of %d" % (head, r["supersteps"], r["supersteps_untrimmed"], r["rows_used"], r["rows"]))
            lines.append("  align call %s = fill %s + walk %s | score call %s kernel %s" % (
                ms(r, "ext_align"), ms(r, "ext_align", "fill_ms"), ms(r, "ext_align", "walk_ms"), ms(r, "ext_score"),
                ms(r, "ext_score", "kernel_ms")))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps({"tool": "align_batch_band_ext_bench", "parts": a.parts, "repeats": a.repeats, "rows": rows}), flush=True)


if __name__ == "__main__":
    main()
