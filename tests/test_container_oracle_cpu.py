"""CPU: the plain references of the container kernels (oracle.ivfpq_oracle get_address_by_id, grow_cells, pack_codes)
checked without the kernels -- against ContainerState's own growth, against the scan layout's formula written out byte
by byte, and on a table small enough to read."""
import numpy as np
import pytest

from oracle import ivfpq_oracle as orc
from torchpq_amd.kernels import PACKED_M


def test_get_address_by_id_on_a_hand_written_table():
    #                  0  1   2  3  4   5  6  7   8  9
    a2i = np.array([7, 3, -1, 9, 3, -1, 7, 0, 3, 12], np.int64)
    ids = np.array([3, 7, 9, 0, 12, 5, -1, -5, 3, 2 ** 62], np.int64)
    want = np.array([1, 0, 3, 7, 9, -1, -1, -1, 1, -1], np.int64)
    got = orc.get_address_by_id(a2i, ids)
    assert got.dtype == np.int64 and np.array_equal(got, want)
    assert np.array_equal(orc.get_address_by_id(a2i, ids.reshape(2, 5)), want.reshape(2, 5))
    assert np.array_equal(orc.get_address_by_id(a2i[:0], ids), np.full(10, -1))
    assert orc.get_address_by_id(a2i, ids[:0]).shape == (0,)
    # an id's answer is an address that holds it, and no smaller address does
    for i, a in zip(ids.tolist(), got.tolist()):
        if a >= 0:
            assert a2i[a] == i and not (a2i[:a] == i).any()
        else:
            assert i < 0 or not (a2i == i).any()


@pytest.mark.parametrize("mode", ["double", "step"])
def test_grow_cells_equals_a_grow_step_of_container_state(mode):
    rng = np.random.default_rng(11)
    m, n_cells = 12, 7
    st = orc.ContainerState(m, n_cells, initial_size=5, expand_step_size=3, expand_mode=mode)
    n = 60
    cells = rng.integers(0, n_cells - 1, n).astype(np.int64)            # the last cell stays empty
    _, adr = st.add(rng.integers(0, 256, (m, n), dtype=np.uint8), cells, rng.permutation(1000)[:n].astype(np.int64))
    st.remove(adr[::4])                                                  # tombstones travel with their cell
    assert (st.is_empty == 0).sum() == n - len(adr[::4]) and (st.storage != 0).any()
    for grown in (np.array([0, 3, 6]), np.array([2]), np.arange(n_cells)):
        old = (st.storage.copy(), st.address2id.copy(), st.is_empty.copy(), st.cell_start.copy(),
               st.cell_capacity.copy())
        st.expand(grown)
        assert (st.cell_capacity[grown] > old[4][grown]).all()
        got = orc.grow_cells(*old, st.cell_start, st.cell_capacity, int(st.cell_capacity.sum()))
        for g, e in zip(got, (st.storage, st.address2id, st.is_empty)):
            assert g.dtype == e.dtype and np.array_equal(g, e)


def test_grow_cells_from_and_to_zero_capacity():
    storage = np.arange(2 * 3 * 4, dtype=np.uint8).reshape(2, 3, 4) + 1
    a2i = np.array([5, -1, 8], np.int64)
    is_empty = np.array([0, 1, 0], np.uint8)
    old_start, old_cap = np.array([0, 0, 2, 3]), np.array([0, 2, 1, 0])
    new_cap = np.array([2, 2, 3, 0])
    new_start = np.cumsum(new_cap) - new_cap
    s, a, e = orc.grow_cells(storage, a2i, is_empty, old_start, old_cap, new_start, new_cap, 7)
    assert a.tolist() == [-1, -1, 5, -1, 8, -1, -1] and e.tolist() == [1, 1, 0, 1, 0, 1, 1]
    assert np.array_equal(s[:, [2, 3, 4]], storage) and not s[:, [0, 1, 5, 6]].any()


def _pack_slowly(storage):
    """the scan layout byte by byte from the header comment of csrc/scan_layout.h: nothing shared with
    orc.pack_codes, not even the block list"""
    g, n_slots, _ = storage.shape
    m = 4 * g
    w = 16 if m % 16 == 0 else 8 if m % 8 == 0 else 4
    out = np.zeros((m // w, n_slots, w), np.uint8)
    for s in range(n_slots):
        p, left = 0, m
        for size in [64] * (m // 64) + [32, 16, 8, 4]:
            if size > left:
                continue
            for r in range(size):                       # position p + r of the block (base p, size)
                j = p + (r ^ (s % size))
                out[(p + r) // w, s, (p + r) % w] = storage[j // 4, s, j % 4]
            p, left = p + size, left - size
        assert left == 0
    return out


@pytest.mark.parametrize("m", sorted(set(PACKED_M) | {4, 12}))
def test_pack_codes_is_the_documented_layout(m):
    rng = np.random.default_rng(m)
    n_slots = 131                                       # past two rounds of the widest block's 64 slot classes
    storage = rng.integers(0, 256, (m // 4, n_slots, 4), dtype=np.uint8)
    packed = orc.pack_codes(storage)
    w = packed.shape[2]
    assert packed.dtype == np.uint8 and packed.shape == (m // w, n_slots, w) and w == max(x for x in (16, 8, 4) if m % x == 0)
    assert np.array_equal(packed, _pack_slowly(storage))
    # the blocks are the greedy powers of two and tile [0, m)
    blocks = orc.scan_layout_blocks(m)
    assert [s for _, s in blocks] == [64] * (m // 64) + [x for x in (32, 16, 8, 4) if (m % 64) & x]
    assert [b for b, _ in blocks] == np.cumsum([0] + [s for _, s in blocks])[:-1].tolist()
    # a slot's permutation is an involution: packing the packed bytes (put back into the storage shape) restores them
    as_storage = np.ascontiguousarray(packed.transpose(0, 2, 1).reshape(m // 4, 4, n_slots).transpose(0, 2, 1))
    assert np.array_equal(orc.pack_codes(as_storage), np.ascontiguousarray(
        storage.transpose(0, 2, 1).reshape(m // w, w, n_slots).transpose(0, 2, 1)))
    # ... and the identity at slot 0 (and at every multiple of 64)
    codes = storage.transpose(0, 2, 1).reshape(m, n_slots)
    at = packed.transpose(0, 2, 1).reshape(m, n_slots)
    assert np.array_equal(at[:, 0], codes[:, 0]) and np.array_equal(at[:, 64], codes[:, 64])
    assert not np.array_equal(at[:, 1], codes[:, 1])
    assert np.array_equal(np.sort(at, axis=0), np.sort(codes, axis=0))


def test_pack_codes_rejects_what_has_no_layout():
    with pytest.raises(AssertionError):
        orc.scan_layout_blocks(6)
    with pytest.raises(AssertionError):
        orc.scan_layout_blocks(0)
