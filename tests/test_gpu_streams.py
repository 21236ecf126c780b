"""Every device entry point on a non-blocking side stream, with inputs that arrive late on that stream.
include/gsa.h promises stream order for every call that takes a `stream`; torch's side streams do not
synchronise with the null stream, so a caller inside `with torch.cuda.stream(s)` depends on it.

Per family (tests/_families.py, Late): the device tensors first hold the decoy inputs; on the stream a
delay is enqueued, then the copies of the true sequences, table and matrices from pinned memory, then an
event; the entry point is called on the stream with nothing synchronised in between, its outputs
prefilled with -7.  A copy, memset, kernel or read-back that the call issues on the null stream or on
another stream of the context sees the decoy or the -7s, and the result differs from the true inputs'
reference (the decoy's result differs: tests/test_families_inputs.py).  For the asynchronous calls the
event must still be pending when the call returns, or the test proves nothing and fails.  (Offset tables
and pair descriptors are host arguments of this API: there is nothing of them to deliver late.)

The delay is calibrated once per session: torch.cuda._sleep(n) timed between two events, n scaled to
about 20 ms and checked to stay under 200 ms.  Measured on the MI355X: 2 398 064 cycles per ms,
n = 47 961 284, which took 19.9 ms (the fixture prints its figures; pytest -s shows them)."""
import pytest

from tests._families import BY_NAME, FAMILIES, SMALL, Late, _n

pytestmark = pytest.mark.gpu

TARGET_MS, LIMIT_MS = 20.0, 200.0
STREAM_FAMILIES = [f for f in FAMILIES if f.takes_stream]


def _timed_sleep(stream, n):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        a.record(stream)
        torch.cuda._sleep(int(n))
        b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


@pytest.fixture(scope="module")
def delay(engine):
    """Cycles of torch.cuda._sleep for about TARGET_MS."""
    import torch
    s = torch.cuda.Stream()
    probe = 2_000_000
    _timed_sleep(s, probe)  # (the first launch loads the kernel)
    ms = _timed_sleep(s, probe)
    assert 0 < ms < LIMIT_MS, ms
    per_ms = probe / ms
    n = int(per_ms * TARGET_MS)
    took = _timed_sleep(s, n)
    print("torch.cuda._sleep: %.0f cycles per ms; n = %d took %.1f ms" % (per_ms, n, took))
    assert TARGET_MS / 2 <= took <= LIMIT_MS, (per_ms, n, took)
    return n


def side_stream(n):
    """A new side stream that the null stream does not wait for.  HIP maps its streams onto a few
    hardware queues (4 by default): a side stream that shares the null stream's queue would run a launch
    mis-issued on the null stream in order behind the delay, and hide it.  So: a tenth of the delay on
    the candidate, then a wait for the null stream, which must come back at once."""
    import time
    import torch
    for _ in range(16):
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            torch.cuda._sleep(n // 10)
        t0 = time.perf_counter()
        torch.cuda.default_stream().synchronize()
        waited = time.perf_counter() - t0
        s.synchronize()
        if waited < 1e-3 * TARGET_MS / 40:
            return s
    raise AssertionError("every side stream shares the null stream's hardware queue")


WARM_RUNS = 4  # the staging rings' slots (csrc/gsa_ctx.h, StageRing::kStage)


def test_no_family_is_left_out():
    assert [f.name for f in FAMILIES if not f.takes_stream] == ["align_sparse", "align_sparse_pt"]  # host-array calls
    assert [f.name for f in FAMILIES if f.asynchronous] == ["fill_sparse", "fill_full", "fill_full_batch", "trace_sparse"]


@pytest.mark.parametrize("family", STREAM_FAMILIES, ids=lambda f: f.name)
def test_late_inputs_on_a_side_stream(engine, delay, family):
    s = side_stream(delay)
    late = Late(s, delay)
    try:
        # first with the inputs in place: the context's buffers grow now (a regrowth frees and allocates,
        # which waits for the device, csrc/gsa_ctx.h reserve), not while the late inputs are pending;
        # an asynchronous call once per slot of the pinned staging rings, which grow slot by slot
        for _ in range(WARM_RUNS if family.asynchronous else 1):
            family.run(engine, SMALL, stream=s.cuda_stream)
        family.run(engine, SMALL, stream=s.cuda_stream, late=late)  # (asserts the result, and the pending event)
        assert late.event is not None
    finally:
        s.synchronize()
    engine.sync(s.cuda_stream)


def test_back_to_back_on_one_stream_then_the_null_stream(engine, delay):
    """Two fills enqueued on the side stream behind late inputs with nothing synchronised between them;
    then, that stream drained (one stream per context at a time), an align call on the null stream.  All
    three results exact."""
    sparse, full = BY_NAME["fill_sparse"], BY_NAME["fill_full"]
    s = side_stream(delay)
    late = Late(s, delay)
    true, decoy = {}, {}
    for tag, f in (("a_", sparse), ("b_", full)):
        for k, v in f.inputs(SMALL)[0]["dev"].items():
            true[tag + k] = v
        for k, v in f.inputs(SMALL, decoy=True)[0]["dev"].items():
            decoy[tag + k] = v
    try:
        for _ in range(WARM_RUNS):  # (the buffers and staging slots grow here, not behind the late inputs)
            sparse.run(engine, SMALL)
            full.run(engine, SMALL)
        t = late.stage(true, decoy)
        _, hr, hc = sparse.launch(engine, {k[2:]: v for k, v in t.items() if k.startswith("a_")}, s.cuda_stream, late)
        out = full.launch(engine, {k[2:]: v for k, v in t.items() if k.startswith("b_")}, s.cuda_stream, late)
        engine.sync(s.cuda_stream)
        assert _n((hr.cpu().numpy(), hc.cpu().numpy())) == sparse.want(SMALL)[0]
        R, C = t["b_y"].numel(), t["b_x"].numel()
        assert _n(out.cpu().numpy().reshape(R, C)) == full.want(SMALL)[0]
        BY_NAME["align_pair"].run(engine, SMALL)
    finally:
        s.synchronize()
