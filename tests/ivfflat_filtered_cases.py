"""The inputs of the IVFFlat filtered-search GPU tests (tests/test_gpu_ivfflat_filtered.py), generated on the CPU so
that tests/test_ivfflat_filtered_cpu.py can assert their conditions on the oracle alone: for each case some query gets
fewer than k results, some query's filtered result differs from its unfiltered top-k, some query has a tie in value across
its k-th place, the sparse filter row leaves a whole tile of the 300-slot cell masked while another tile of it has a hit,
and -- by a model of the masked scan's walk (walk()) -- under the sparse row some wave is left with pending slots to
drain after its last tile, under the `half` row some wave values partial tiles in place, and in the cases with a cell
of 40 000 slots some wave under the sparse row owns enough sparse tiles to carry it past 64 pending slots WITH a
remainder left to drain.  (The scan compacts only tiles with fewer than COMPACT_BELOW live slots -- measured, DESIGN
3.15 -- so the `half` row, 32 live slots a tile, never fills a pending list; the long cell is what does.)

The inverted lists are those of tests/test_gpu_ivfflat._case -- cells of 0, 1, 63, 64, 65, 300, 17 and 128 slots with
spare capacity behind each, tombstones, planted duplicate vectors, a cell listed twice, n_probe_list below, at and
beyond max_nprobe -- with one cell of 1 500 slots more (24 tiles: three per wave) and seeds whose capacity is not a
multiple of 32.  The kernel takes ONE mask per launch, so a run is a filter row applied to every query.

The value of a slot does not depend on the mask: the candidates of a case are valued once, without a mask
(ivfflat_range_oracle.candidates), and every row only selects among them.  tests/test_ivfflat_filtered_cpu.py checks
that this is ivfflat_filtered_oracle.scan_topk.
"""
import functools

import numpy as np

import ivfflat_oracle as forc
import ivfflat_range_oracle as rorc
from test_gpu_ivfflat import CELL_SIZES, _case

SIZES = CELL_SIZES + (1500,)
KS = (1, 10, 100, 1024)
SPLITS = (None, 1, 5, 7)
ROWS = ("ones", "zeros", "single", "sparse", "half")
N_WAVES = 8          # waves of a scan workgroup: wave w of a part takes the part's tiles w, w + 8, ...
COMPACT_BELOW = 4    # kCompactBelow of csrc/scan_flat.hip: a partial tile with fewer live slots than this is compacted
LONG_CELL = 40000    # 625 tiles, 78 a wave: at 3 % allowed about a hundred pending slots per wave

# (d, nq, n_probe, distance, long): every d (below, at and above the unroll of eight rows, and its tail), every nq, both
# metrics per d; d = 960 with at most three queries; `long`: the layout has a cell of LONG_CELL slots too
KERNEL_CASES = [
    (1, 3, 8, "euclidean", False),
    (1, 1000, 4, "inner", False),
    (3, 1, 8, "inner", True),
    (3, 1000, 8, "euclidean", False),
    (24, 3, 8, "euclidean", True),
    (24, 1000, 1, "inner", False),
    (128, 1, 8, "euclidean", False),
    (128, 1000, 4, "euclidean", False),
    (128, 3, 8, "inner", True),
    (960, 3, 8, "euclidean", False),
    (960, 1, 8, "inner", False),
]


def metric(distance):
    return "euclidean" if distance == "euclidean" else "inner"


def filter_rows(case, rng):
    """allowed bool [5, capacity] (ROWS) and the start of the 300-slot cell, or None when the layout cannot carry them.
    Every row also allows the tombstones and the free slots between the cells: none of these may produce a hit."""
    is_empty = case["is_empty"]
    cap = len(is_empty)
    at = np.argwhere(case["sz"] == 300)
    if len(at) == 0:
        return None
    start = int(case["cs"][at[0][0], at[0][1]])
    live = is_empty == 0
    slots = np.arange(cap)
    tile = lambda t: np.flatnonzero(live & (slots >= start + 64 * t) & (slots < min(start + 64 * t + 64, start + 300)))
    if len(tile(0)) == 0 or len(tile(2)) == 0:
        return None
    rows = np.zeros((len(ROWS), cap), bool)
    rows[0] = True
    rows[2, rng.choice(tile(2))] = True
    rows[3] = rng.random(cap) < 0.03
    rows[3, start + 64:start + 128] = False          # tile 1 of the 300-slot cell: nothing allowed
    rows[3, rng.choice(tile(0))] = True              # tile 0: at least one hit
    rows[4] = rng.random(cap) < 0.5
    rows[1:] &= live
    rows |= ~live
    return rows, start


def masks_of(case):
    """u8 [5, capacity]: what the kernel is handed for each row, `is_empty | ~allowed[row]`"""
    return ((case["is_empty"] != 0)[None, :] | ~case["allowed"]).astype(np.uint8)


def query_tiles(cell_start, cell_size, n_probe, capacity):
    """the 64-slot tiles one query scans, in scan order, each as the slots of it inside the cell and the storage (the
    probes are ivfflat_oracle.probed_slots')"""
    out, max_nprobe = [], len(cell_start)
    for p in range(min(max(int(n_probe), 0), max_nprobe)):
        st, sz = int(cell_start[p]), int(cell_size[p])
        if sz <= 0 or (p > 0 and int(cell_start[p - 1]) == st):
            continue
        for lo in range(0, sz, 64):
            s = np.arange(st + lo, st + min(lo + 64, sz), dtype=np.int64)
            out.append(s[(s >= 0) & (s < capacity)])
    return out


def walk(mask, tiles, n_split=1):
    """A model of the masked scan's documented walk (csrc/scan_flat.hip): part i of n_split takes the tiles
    [total i / n_split, total (i + 1) / n_split), wave w of it every eighth from its w-th on; a tile without a live
    slot is skipped, one whose every slot is live is valued in place, and so is a partial tile with COMPACT_BELOW live
    slots or more (`partial`); a sparser one (`sparse`) appends its live slots to the wave's pending list, which gives
    64 away whenever it holds 64 or more.  -> per (part, wave) a dict of counts: skipped, full, partial, sparse, takes,
    and `left`, what is drained after the wave's last tile."""
    total, out = len(tiles), []
    for part in range(n_split):
        lo, hi = total * part // n_split, total * (part + 1) // n_split
        for w in range(N_WAVES):
            c = dict(part=part, wave=w, skipped=0, full=0, partial=0, sparse=0, takes=0, left=0)
            for T in range(lo + w, hi, N_WAVES):
                live = int((mask[tiles[T]] == 0).sum())
                if live == 0:
                    c["skipped"] += 1
                elif live == len(tiles[T]):
                    c["full"] += 1
                elif live >= COMPACT_BELOW:
                    c["partial"] += 1
                else:
                    c["sparse"] += 1
                    c["left"] += live
                    assert c["left"] < 128           # the list has 128 places
                    if c["left"] >= 64:
                        c["left"] -= 64
                        c["takes"] += 1
            out.append(c)
    return out


def topk_many(cand, ks):
    """per-query candidates (slots, values) -> {k: (values f32 [nq, k], address i64 [nq, k])}: value descending,
    address ascending, NaN removed, (-inf, -1) pads -- one sort per query for every k"""
    nq = len(cand)
    out = {k: (np.full((nq, k), -np.inf, np.float32), np.full((nq, k), -1, np.int64)) for k in ks}
    for q, (s, v) in enumerate(cand):
        keep = ~np.isnan(v)
        s, v = s[keep], v[keep]
        order = np.lexsort((s, -v.astype(np.float64)))
        for k in ks:
            o = order[:k]
            out[k][0][q, :len(o)] = v[o]
            out[k][1][q, :len(o)] = s[o]
    return out


def select(cand, mask):
    """the candidates a mask leaves"""
    return [(s[mask[s] == 0], v[mask[s] == 0]) for s, v in cand]


def conditions(case):
    """the conditions of the module docstring, on the oracle's results alone -> dict of bools"""
    plain = case["cand"][0]                            # row 0 skips the tombstones only: the unfiltered scan
    fewer = differs = tie = False
    for cand in case["cand"][1:]:
        for (s, v), (us, uv) in zip(cand, plain):
            n = int((~np.isnan(v)).sum())
            order = np.lexsort((s, -v.astype(np.float64)))
            uorder = np.lexsort((us, -uv.astype(np.float64)))
            for k in KS:
                fewer |= n < k
                differs |= not np.array_equal(s[order][:k], us[uorder][:k])
                tie |= n > k and v[order][k - 1] == v[order][k]
    start, sparse = case["big_start"], case["masks"][3] == 0
    tiles300 = [sparse[start + 64 * t:min(start + 64 * t + 64, start + 300)].any() for t in range(5)]
    seen = any(((s >= start) & (s < start + 300)).any() for s, _ in case["cand"][3])
    cap = len(case["is_empty"])
    drained = taken = in_place = False
    for q in range(case["cs"].shape[0]):
        tiles = query_tiles(case["cs"][q], case["sz"][q], case["npl"][q], cap)
        sparse_walk, half_walk = walk(case["masks"][3], tiles), walk(case["masks"][4], tiles)
        drained |= any(w["left"] > 0 for w in sparse_walk)
        taken |= any(w["takes"] >= 1 and w["left"] > 0 for w in sparse_walk)
        in_place |= any(w["partial"] > 0 for w in half_walk)
    return dict(fewer=fewer, differs=differs, tie=tie, masked_tile=(not tiles300[1]) and tiles300[0], sparse_seen=seen,
                drain=drained, partial_in_place=in_place, take_and_drain=taken or not case["long"])


@functools.lru_cache(maxsize=None)
def kernel_case(d, nq, n_probe, distance, long=False):
    """the first seed whose layout has a capacity that is no multiple of 32, carries the filter rows and meets
    conditions(); the oracle's results for every row and k, computed once"""
    seed0 = 4000 * d + 10 * nq + n_probe
    for seed in range(seed0, seed0 + 200):
        case = _case(seed, d, nq, n_probe, sizes=SIZES + ((LONG_CELL,) if long else ()),
                     scale=0.25 if d >= 960 else 1.0)
        if len(case["is_empty"]) % 32 == 0:
            continue
        rows = filter_rows(case, np.random.default_rng(seed + 1))
        if rows is None:
            continue
        case.update(seed=seed, allowed=rows[0], big_start=rows[1], long=long)
        case["masks"] = masks_of(case)
        every = rorc.candidates(case["vectors"], case["query"], None, case["cs"], case["sz"], case["npl"],
                                metric(distance))
        case["cand"] = [select(every, mask) for mask in case["masks"]]
        if all(conditions(case).values()):
            case["want"] = {}
            for r, cand in enumerate(case["cand"]):
                for k, res in topk_many(cand, KS).items():
                    case["want"][r, k] = res
            return case
    raise AssertionError("no seed gives a case that meets its conditions")
