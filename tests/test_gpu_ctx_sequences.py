"""Call-order independence on one context: every entry-point family (tests/_families.py) right after every
other one, and after calls that leave something behind on purpose, on one fresh engine.  The context's
grow-only buffers and control words are shared by all calls (csrc/gsa_ctx.h, BufId; DESIGN.md 2.2, "What
the calls share"): the hand-off granules, the 64 bytes of score control words, the pair and database
trace slots, the descriptor and staging rings, the ticket / error / q8 words and the epoch.  A stale
control word, a granule read under another layout, a walk record left in a slot or an error bit that
leaks into the next gsa_sync shows as a result of B that differs after some predecessor A.

Every run is checked against the CPU references by the family's runner; B's result is also compared
with its first one for identity."""
import pytest

import gpuseqalign_amd as gsa
from tests._families import DIRTY, FAMILIES, SIZES, SMALL

pytestmark = pytest.mark.gpu


@pytest.fixture
def fresh():
    """make(): a new engine, closed after the test."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    made = []

    def make():
        made.append(gsa.Engine(0))
        return made[-1]

    yield make
    for e in made:
        e.close()


def predecessors():
    """(name, run(e)) of every family, small and large alternating down the list, then the dirty ones."""
    out = []
    for k, f in enumerate(FAMILIES):
        size = SIZES[k % 2]
        out.append(("%s-%s" % (f.name, size), lambda e, f=f, size=size: f.run(e, size)))
    return out + [(d.name, d.run) for d in DIRTY]


@pytest.mark.parametrize("B", FAMILIES, ids=lambda f: f.name)
def test_after_every_predecessor(fresh, B):
    """B alone, then A, B, gsa_sync for every predecessor A: B's result is the first one every time (and
    the reference's: the runner asserts that), and gsa_sync reports nothing."""
    e = fresh()
    first = B.run(e, SMALL)
    e.sync()
    for name, run in predecessors():
        print(B.name, "after", name)  # (pytest shows it when the test fails: the last predecessor)
        run(e)
        got = B.run(e, SMALL)
        assert got == first, (B.name, "after", name)
        e.sync()


MODE_FAMILIES = [f for f in FAMILIES if len(f.modes(SMALL)) > 1]


@pytest.mark.parametrize("family", MODE_FAMILIES, ids=lambda f: f.name)
def test_same_family_changes_mode(fresh, family):
    """One family through its modes and back on one context: affine, linear, local where the call has it,
    affine again (the granule layout differs by mode: gran, gran2).  The score calls on the K-rows kernel
    also with 2, 4 and 2 rows per lane (the layout differs by K) and with the 8-bit profile off, on and
    off."""
    e = fresh()
    n = len(family.modes(SMALL))
    there_and_back = list(range(n)) + [0]
    first = family.run(e, SMALL, order=there_and_back)
    assert first[-1] == first[0]
    if not family.krow_score:
        return
    for knob, values in [("GSA_SCORE_K", ("2", "4", "2")), ("GSA_KROW_Q8", ("0", "1", "0"))]:
        for v in values:
            e.set_knob(knob, v)
            print(family.name, knob, v)
            assert family.run(e, SMALL, order=there_and_back) == first, (family.name, knob, v)
            e.sync()
        e.set_knob(knob, None)
    assert family.run(e, SMALL, order=there_and_back) == first
