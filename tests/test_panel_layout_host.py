"""The panel layout of the solve tiles (dpgo_amd/csrc/spd_panel.h) as the host packer of SpdSolverDev::upload applies it,
through dpgo_debug_spd_panel_pack (no GPU).

A tile's lane (r, kq), KQ = 64 / rows lanes per row, consumes the entries k = kq, kq + KQ, ... of its row r.  In the paired
layout (KQ = 1 and 4: the 64- and 16-row classes) entry (k, r), k = g 2KQ + h KQ + kq, lies at ((g KQ + kq) ld + r) 2 + h, so
the two halves of a 16-byte unit are (k, r) and (k + KQ, r), and the panel's length in k is rounded up to a multiple of 2 KQ.
The 8-row root class (KQ = 8) keeps the plain layout (k ld + r) whatever the switch says: chunks of the reduction start at
multiples of 8 and a pair group would take 16.  The source entry (k, r) holds 1000 k + r: every entry but (0, 0), which is
the panel's first double in either layout, is told from the zeros of the padding by its value."""
import itertools

import numpy as np
import pytest

import dpgo_amd

KQS = (1, 4, 8)
COUNTS = (1, 15, 16, 17, 64)
LENS = (1, 2, 7, 8, 9, 15, 16, 17, 129)
CASES = [(kq, c, n) for kq, c, n in itertools.product(KQS, COUNTS, LENS) if c <= 64 // kq]


def source(count, length):
    k, r = np.meshgrid(np.arange(length), np.arange(count), indexing="ij")
    return 1000.0 * k + r


def test_every_size_of_the_list_occurs_for_some_class():
    assert {c for _, c, _ in CASES} == set(COUNTS) and {n for _, _, n in CASES} == set(LENS)
    assert {kq for kq, _, _ in CASES} == set(KQS)


@pytest.mark.parametrize("pairs", [True, False])
@pytest.mark.parametrize("kq,count,length", CASES)
def test_panel(kq, count, length, pairs):
    rows = 64 // kq
    src = source(count, length)
    mat_off = 48   # (16-byte aligned, as every panel's offset is)
    panel, info = dpgo_amd.spd_panel_pack_debug(src, rows, pairs=pairs, mat_off=mat_off)
    paired = pairs and kq in (1, 4)
    ld = 8 if rows == 8 else (count + 15) // 16 * 16
    # what the item reports: row distance, layout, offset; the panel's length; 16-byte alignment of it and of what follows
    assert info["ld"] == ld and info["pair_kq"] == (kq if paired else 0) and info["mat_off"] == mat_off
    padded = -(-length // (2 * kq)) * (2 * kq) if paired else length
    assert info["doubles"] == padded * ld and panel.size == mat_off + padded * ld
    assert (8 * info["mat_off"]) % 16 == 0 and (8 * (info["mat_off"] + info["doubles"])) % 16 == 0
    assert not panel[:mat_off].any()
    body = panel[mat_off:]
    # a bijection of the entries into the panel; every other entry is zero
    nz = np.union1d(np.flatnonzero(body), [0])
    assert nz.size == count * length
    assert np.array_equal(np.sort(body[nz]), np.sort(src.ravel()))
    # where each entry is
    k, r = np.meshgrid(np.arange(length), np.arange(count), indexing="ij")
    if paired:
        g, rem = k // (2 * kq), k % (2 * kq)
        h, q = rem // kq, rem % kq
        where = ((g * kq + q) * ld + r) * 2 + h
    else:
        where = k * ld + r
    assert np.array_equal(body[where], src)
    if paired:
        # the two halves of a 16-byte unit: (k, r) and (k + KQ, r), or a zero of the padding where k + KQ is past the end
        units = body.reshape(-1, 2)
        used = np.union1d(np.flatnonzero(units.any(axis=1)), [0])
        assert used.size == np.count_nonzero((k % (2 * kq)) < kq)
        for u in used:
            x, y = units[u]
            assert x != 0.0 or u == 0
            kx, rx = int(x) // 1000, int(x) % 1000
            assert (kx % (2 * kq)) < kq and rx < count
            assert y == (1000.0 * (kx + kq) + rx if kx + kq < length else 0.0)


@pytest.mark.parametrize("kq,count,length", [(1, 17, 9), (4, 15, 17), (8, 1, 7)])
def test_the_packer_writes_the_entries_and_nothing_else(kq, count, length):
    src = source(count, length)
    panel, info = dpgo_amd.spd_panel_pack_debug(src, 64 // kq, pairs=True, mat_off=16, fill=-7.0)
    assert np.count_nonzero(panel != -7.0) == count * length


def test_bad_arguments_are_refused():
    with pytest.raises(ValueError):
        dpgo_amd.spd_panel_pack_debug(source(17, 4), 16)   # (more rows than the class has)
    with pytest.raises(ValueError):
        dpgo_amd.spd_panel_pack_debug(source(4, 4), 32)    # (no such class)
