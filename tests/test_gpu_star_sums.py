"""AMM-PGO*'s master sums on the device -- k_star_sums, k_publish -- on GIVEN partial sums (NodeGroup.debug_star_sums: the two
launches Group::star_sums ends with, with its slot table) against a restatement:

  s_q(a) = the sum of node a's partials in slot SLOTS[q] over its own segments and, for q < 4, its neighbour segments
  F1 = sum_a 1/2 s_0(a) + 1/4 s_1(a),  F2 = sum_a 1/2 s_2(a) + 1/4 s_3(a),  d1 = sum_a s_4(a),  d2 = sum_a s_5(a)

with a sum whose bit in `valid` is off counting as zero.  Exact inputs (small integers times powers of two, split unevenly
over the segments: every order of summation gives the same double) must come out exactly, under every one of the 64 masks;
what must not be read holds NaN: the slots whose bit is off, the neighbour segments of slots 4 and 5, every slot outside the
six.  One random input is held to (ceil(nseg / 64) + 6 + nnodes + 2) u sum |terms| around math.fsum -- a node's lane loop, the
six levels of wave_sum, the sum over the nodes, the two products and the add of a node's term -- and to the same bits in
three launches.  k_publish: the pinned values are the device values bit for bit, the flag is the last sequence number.

Groups: synthetic.ladder(3) (6 nodes) and the one-node synthetic.grid(17, 17, 16) (73 own segments, no neighbour).
"""
import math
from fractions import Fraction

import numpy as np
import pytest

from test_gpu_cg_scalars import ladder_group, wide_group   # noqa: F401  (fixtures)
from test_gpu_gate import place, _bits

NAN = float("nan")
MAX_SLOTS = 32
SLOTS = (0, 1, MAX_SLOTS - 2, MAX_SLOTS - 1, 4, 5)     # Group::star_sums
WEIGHT = (0.5, 0.25, 0.5, 0.25, 1.0, 1.0)


def exact_table(layout, valid):
    """-> (the table, the four values).  own(q, a) = (a + 1)(q + 2) / 4, nbr(q, a) = -(a + 2)(q + 1) / 8"""
    nseg_all, own, nbr = layout
    L = len(own) - 1
    T = np.full((MAX_SLOTS, nseg_all), NAN)
    want = [Fraction(0)] * 4
    for q, s in enumerate(SLOTS):
        if not (valid >> q) & 1:
            continue                                   # (the slot keeps its NaN)
        for a in range(L):
            v = (a + 1) * (q + 2) * 0.25
            T[s, own[a]:own[a + 1]] = place(v, own[a + 1] - own[a], a + q)
            n = nbr[a + 1] - nbr[a]
            w = -(a + 2) * (q + 1) * 0.125 if (q < 4 and n > 0) else 0.0
            if q < 4 and n > 0:
                T[s, nbr[a]:nbr[a + 1]] = place(w, n, a)
            want[q // 2 if q < 4 else q - 2] += Fraction(WEIGHT[q]) * (Fraction(v) + Fraction(w))
    return T, [float(x) for x in want]


def test_the_exact_table_is_exact():
    layout = (9, np.array([0, 1, 3, 6]), np.array([6, 7, 9, 9]))
    T, want = exact_table(layout, 0x3f)
    assert not np.isnan(T[list(SLOTS[:4])]).any() and np.isnan(T[4, 6:]).all() and np.isnan(T[2]).all()
    # F1 = sum_a 1/2 (a + 1) 2/4 - 1/2 (a + 2) / 8 + 1/4 (a + 1) 3/4 - 1/4 (a + 2) 2/8, the third node without neighbours
    assert want[0] == sum(0.25 * (a + 1) + 0.1875 * (a + 1) - (0.125 * (a + 2) if a < 2 else 0.0) for a in range(3))
    assert want[2] == sum((a + 1) * 1.5 for a in range(3))


def check(group, T, valid, want=None, before=None):
    grp, layout = group
    o = grp.debug_star_sums(T, valid)
    assert np.array_equal(_bits(o["host"]), _bits(o["dev"])), (valid, o)        # k_publish
    assert o["flag"] == o["seq"] and (before is None or o["seq"] == before["seq"] + 1)
    if want is not None:
        assert np.array_equal(_bits(o["dev"]), _bits(want)), (bin(valid), o["dev"], want)
    return o


@pytest.mark.gpu
def test_every_valid_mask(ladder_group):
    grp, layout = ladder_group
    assert np.all(np.diff(layout[2]) > 0)      # every node of the ladder has neighbour segments
    o = None
    for valid in range(64):
        T, want = exact_table(layout, valid)
        o = check(ladder_group, T, valid, want, o)


@pytest.mark.gpu
def test_one_node_of_73_segments(wide_group):
    for valid in (0x3f, 0x15, 0x2a, 0):
        T, want = exact_table(wide_group[1], valid)
        check(wide_group, T, valid, want)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["ladder", "wide"])
def test_random_sums(ladder_group, wide_group, which):
    group = ladder_group if which == "ladder" else wide_group
    nseg_all, own, nbr = group[1]
    L = len(own) - 1
    rng = np.random.default_rng(13)
    T = rng.standard_normal((MAX_SLOTS, nseg_all)) * np.exp2(rng.integers(-10, 10, (MAX_SLOTS, 1)))
    T[[s for s in range(MAX_SLOTS) if s not in SLOTS]] = NAN
    for a in range(L):
        T[4:6, nbr[a]:nbr[a + 1]] = NAN
    o = check(group, T, 0x3f)
    for _ in range(2):
        again = check(group, T, 0x3f, before=o)
        assert np.array_equal(_bits(again["dev"]), _bits(o["dev"]))
        o = again
    nseg = max((own[a + 1] - own[a]) + (nbr[a + 1] - nbr[a]) for a in range(L))
    factor = (math.ceil(nseg / 64) + 6 + L + 2) * 2.0 ** -53
    for k in range(4):
        terms = []
        for q in ((2 * k, 2 * k + 1) if k < 2 else (k + 2,)):
            for a in range(L):
                terms += list(WEIGHT[q] * T[SLOTS[q], own[a]:own[a + 1]])
                if q < 4:
                    terms += list(WEIGHT[q] * T[SLOTS[q], nbr[a]:nbr[a + 1]])
        assert abs(o["dev"][k] - math.fsum(terms)) <= factor * math.fsum(abs(x) for x in terms), (k, o["dev"][k])
