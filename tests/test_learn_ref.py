"""tests/learn_ref.py (the model the device learning is compared with,
tests/test_gpu_learn.py) against properties stated independently of it: the
order is a permutation with the documented ties, the heavy-pixel bar is the
exact rational up to its three double roundings, the XCD grouping deals the
eighths of a brute-force ranking.  Also the synthetic learning inputs the GPU
test feeds the kernels (synth, cases), with the properties they must have
asserted here, before a GPU is touched."""
import math
from fractions import Fraction

import numpy as np
import pytest

import learn_ref as L

RESIDENT = 6144                 # 256 CUs x 24 resident waves: no power of two
NS = (1, 8, 63, 64, 65, 257, 1000)
FACTORS = (10, 30, 50, 75, 100, 130)
SEARCHED = FACTORS + (15, 35, 60, 70, 120)     # heavy_pixel_factor values searched for bar disagreements


def scaled_bar(total, factor, concurrent, resident):
    """The pre-multiplied form the device kernel used: (factor/100 x
    concurrent / resident) x total.  Not the contract; kept to find inputs at
    which it and the host's form (learn_ref.heavy_bar) disagree."""
    return (factor / 100.0 * float(concurrent) / float(resident)) * float(total)


def bar_triples(per_pair=2, k_max=400):
    """(factor, concurrent, total, length): a pixel of that walk length is
    heavy under exactly one of the two bar formulas."""
    out = []
    for f in SEARCHED:
        for c in (1, 4):
            found = 0
            for k in range(1, k_max):
                total = RESIDENT * k
                new, old = L.heavy_bar(total, f, c, RESIDENT), scaled_bar(total, f, c, RESIDENT)
                n = math.ceil(min(new, old))
                if new != old and (n > new) != (n > old):
                    out.append((f, c, total, n))
                    found += 1
                    if found == per_pair:
                        break
    return out


def _split_cost(rng, cost):
    """words 4, 5 with w4 + 2 w5 = cost"""
    w5 = int(rng.randint(0, min(cost // 2, 1 << 20) + 1))
    return cost - 2 * w5, w5


def synth(n, seed, *, kind="ties", learn_cost=0, rec_off=0, order_split=0, factor=50, concurrent=1,
          resident=RESIDENT, cap="above", xcd=0, grid=(0, 0, 0), total=None, length=None):
    """A learning launch's records and lanes, and learn()'s keyword arguments.
    kind: "ties" (costs from a few levels, one of them exactly order_split% of
    the costliest; lengths around the bar), "zero" (all-zero costs), "big"
    (costs at and past 2^32, a wrapped duration), "none" (no pixel over the
    bar), "all" (every pixel over it), "bar" (steps summing to `total`, pixels
    of `length` and its neighbours).  cap: "below" / "equal" / "above" the
    candidate count, or a number."""
    rng = np.random.RandomState(seed)
    rec = rng.randint(0, 1 << 62, size=(rec_off + n, 8), dtype=np.int64).astype(np.uint64)   # junk everywhere
    rec[:rec_off] |= np.uint64(1 << 63)
    levels = [0, 7, 199, 200, 201, 640, 1000, 1000]
    if kind in ("ties", "none", "all"):
        cost = [int(c) for c in rng.choice(levels, n)]
        if n >= 8:
            cost[n // 2], cost[n - 1], cost[1], cost[2] = 1000, 1000, 200, 199
    elif kind == "zero":
        cost = [0] * n
    elif kind == "bar":
        cost = [total // n] * n
        cost[0] += total - sum(cost)
    else:   # big: tile 0 small, so the raster order is not the answer
        big = [2 ** 32 - 1, 2 ** 32, 2 ** 32 + 5, 2 ** 40, 2 ** 32 - 2, 3, 2 ** 31]
        cost = [5] + [int(big[i]) for i in rng.randint(0, len(big), n - 1)]
        if n >= 8:
            cost[3], cost[5], cost[6] = 2 ** 40, 2 ** 32 - 1, 2 ** 32 - 2
    for k in range(n):
        r = rec[rec_off + k]
        if learn_cost == 0:
            r[4], r[5] = _split_cost(rng, cost[k])
        else:
            r[0] = int(rng.randint(0, 1 << 40))
            r[1] = int(r[0]) + cost[k]
            steps = 0 if kind == "zero" else (cost[k] if kind == "bar" else int(rng.randint(0, 1200)))
            r[4], r[5] = _split_cost(rng, steps)
    if kind == "big" and learn_cost == 1 and n >= 8:
        rec[rec_off + 4, 0], rec[rec_off + 4, 1] = 1000, 10          # the counter wrapped: cost 2^64 - 990
    steps, _ = L.tile_costs(rec.tolist(), rec_off, learn_cost)
    bar = L.heavy_bar(sum(steps), factor, concurrent, resident)
    nl = 64 * n
    if kind == "none":
        lane = rng.randint(0, int(bar) + 1, nl)
    elif kind == "all":
        lane = rng.randint(int(bar) + 1, int(bar) + 4, nl)
        lane[rng.randint(0, nl, 3)] = 0x3FFFFFFF                     # a heavy wave's mark (kLearnHeavyMark)
    elif kind == "bar":
        lane = rng.choice([0, max(length - 1, 0), length, length + 1], nl, p=[0.7, 0.1, 0.1, 0.1])
        lane[:3] = (length, max(length - 1, 0), length + 1)
    else:
        lane = np.where(rng.rand(nl) < 0.1, rng.randint(int(bar), int(bar) + 5, nl), rng.randint(0, int(bar) + 2, nl))
    lane = lane.astype(np.uint32)
    n_cand = int((lane.astype(np.float64) > bar).sum())
    cap_n = {"below": n_cand // 2, "equal": n_cand, "above": n_cand + 7}.get(cap, cap)
    kw = dict(rec_off=rec_off, learn_cost=learn_cost, order_split=order_split, heavy_pixel_factor=factor,
              concurrent=concurrent, resident=resident, cap=int(cap_n), xcd=xcd, tiles_x=grid[0], tiles_y=grid[1],
              frames=grid[2])
    return dict(n=n, kind=kind, records=rec, lane=lane, kw=kw, n_cand=n_cand, bar=bar)


def want(case):
    return L.learn(case["records"].tolist(), case["lane"].tolist(), **case["kw"])


# (tiles_x, tiles_y, frames) per tile count; 63, 65 and 257 tiles are no multiple of 8: the plain order
GRIDS = {8: [(1, 8, 1), (2, 1, 4), (1, 2, 4)], 64: [(4, 16, 1), (2, 8, 4), (8, 8, 1), (1, 64, 1)],
         1000: [(5, 50, 4), (10, 25, 4), (25, 40, 1), (4, 250, 1)], 63: [(9, 7, 1)], 65: [(13, 5, 1)],
         257: [(257, 1, 1)]}


def cases():
    """name -> synth() keyword arguments: every input of tests/test_gpu_learn.py."""
    out = {}
    for i, n in enumerate(NS):
        for lc in (0, 1):
            for j, split in enumerate((0, 20, 100)):
                out[f"ties-n{n}-c{lc}-s{split}"] = dict(n=n, seed=100 * i + 10 * lc + j, learn_cost=lc,
                                                        rec_off=(0, 5)[(i + lc + j) % 2], order_split=split,
                                                        cap=("below", "equal", "above")[(i + j) % 3],
                                                        concurrent=(1, 4)[(i + lc) % 2])
            out[f"big-n{n}-c{lc}-s100"] = dict(n=n, seed=900 + 10 * i + lc, kind="big", learn_cost=lc, order_split=100,
                                               rec_off=5 * lc)
            out[f"big-n{n}-c{lc}-s20"] = dict(n=n, seed=950 + 10 * i + lc, kind="big", learn_cost=lc, order_split=20,
                                              cap="equal")
        out[f"big-n{n}-c0-s0"] = dict(n=n, seed=980 + i, kind="big", order_split=0, cap="below")
        out[f"zero-n{n}"] = dict(n=n, seed=700 + i, kind="zero", learn_cost=i % 2, order_split=(0, 20, 100)[i % 3])
        out[f"none-n{n}"] = dict(n=n, seed=710 + i, kind="none", cap=(5, 0)[i % 2])
        out[f"all-n{n}"] = dict(n=n, seed=720 + i, kind="all", cap=(64 * n, 64 * n + 9, 3)[i % 3], factor=130)
        for g, grid in enumerate(GRIDS.get(n, [])):
            for xcd in (1, 2, 3):
                out[f"xcd{xcd}-n{n}-{'x'.join(map(str, grid))}"] = dict(
                    n=n, seed=800 + 10 * i + g, xcd=xcd, grid=grid, order_split=(0, 20)[(g + xcd) % 2],
                    learn_cost=(g + xcd) % 2, rec_off=5 * (g % 2))
    out["xcd2-n1000-grid-mismatch"] = dict(n=1000, seed=899, xcd=2, grid=(10, 50, 1))
    for t, (f, c, total, length) in enumerate(bar_triples()):
        out[f"bar-f{f}-c{c}-t{total}"] = dict(n=NS[t % len(NS)], seed=600 + t, kind="bar", factor=f, concurrent=c,
                                              total=total, length=length, learn_cost=t % 2, cap=10 ** 6)
    return out


CASES = cases()


@pytest.fixture(scope="module")
def built():
    """Every case and the model's answer for it, computed once."""
    out = {}
    for name, kw in CASES.items():
        c = synth(**kw)
        out[name] = (c, want(c))
    return out


def test_the_bar_is_the_exact_rational_up_to_its_roundings():
    # every operation exact: factor/100 a dyadic rational, a power-of-two resident count
    for f, c, total, res in ((50, 1, 12345, 4096), (75, 4, 999, 1024), (25, 3, 1 << 40, 1 << 12), (200, 1, 7, 1)):
        assert Fraction(L.heavy_bar(total, f, c, res)) == Fraction(f, 100) * total * c / res
    # otherwise three roundings (quotient, the constant factor/100, the product), each 2^-53 relative
    rng = np.random.RandomState(1)
    for _ in range(2000):
        f, c = int(rng.choice(FACTORS)), int(rng.choice([1, 2, 4]))
        total, res = int(rng.randint(1, 1 << 40)), int(rng.choice([RESIDENT, 304 * 24, 64 * 24]))
        exact = Fraction(f, 100) * total * c / res
        assert abs(Fraction(L.heavy_bar(total, f, c, res)) - exact) <= exact * Fraction(3, 2 ** 53) * Fraction(101, 100)
    # the documented case: the host's bar is 3 exactly, the pre-multiplied form falls below it
    assert L.heavy_bar(61440, 30, 1, RESIDENT) == 3.0 and scaled_bar(61440, 30, 1, RESIDENT) == 2.9999999999999996
    assert max(1, 0) == 1 and L.heavy_bar(10, 50, 0, 0) == 5.0           # concurrency and residents are at least 1
    triples = bar_triples()
    assert (30, 1, 61440, 3) in triples
    assert {f for f, *_ in triples} >= {30, 15, 35, 60, 70, 120} and 50 not in {f for f, *_ in triples}
    assert {c for _, c, *_ in triples} == {1, 4} and len(triples) >= 12
    for f, c, total, length in triples:
        assert (length > L.heavy_bar(total, f, c, RESIDENT)) != (length > scaled_bar(total, f, c, RESIDENT))


def test_costs_and_keys():
    rec = [[10, 4, 0, 0, 7, 3, 0, 0], [5, 2 ** 33 + 5, 0, 0, 2 ** 32, 1, 0, 0], [9, 9, 9, 9, 9, 9, 9, 9]]
    assert L.tile_costs(rec, 0, 0) == ([13, 2 ** 32 + 2, 27], [13, 2 ** 32 + 2, 27])
    assert L.tile_costs(rec, 1, 1) == ([2 ** 32 + 2, 27], [2 ** 33, 0])
    assert L.tile_costs(rec, 0, 1)[1][0] == 2 ** 64 - 6                 # a wrapped duration
    # costs past the key's range tie: raster order among them, ahead of everything else
    assert L.cost_order([5, 2 ** 32 - 1, 2 ** 40, 2 ** 32 - 2, 2 ** 64 - 6], 0) == [1, 2, 4, 3, 0]
    assert L.cost_order([5, 2 ** 32 - 1, 2 ** 40, 2 ** 32 - 2, 2 ** 64 - 6], 100) == [1, 2, 4, 0, 3]
    # the split: at the threshold is in, below it keeps raster order
    assert L.cost_order([1, 199, 1000, 200, 3, 1000, 640], 20) == [2, 5, 6, 3, 0, 1, 4]
    assert L.cost_order([1, 199, 1000, 200, 3, 1000, 640], 100) == [2, 5, 0, 1, 3, 4, 6]
    assert L.cost_order([0, 0, 0], 0) == L.cost_order([0, 0, 0], 100) == [0, 1, 2]
    assert L.cost_order([3, 0, 3, 9, 0], 0) == [3, 0, 2, 1, 4]


def test_heavy_pixels_order_and_cap():
    lane = [0, 5, 9, 5, 3, 9, 2, 5]
    assert L.heavy_pixels(lane, 2.5, 100) == [2, 5, 1, 3, 7, 4]
    assert L.heavy_pixels(lane, 2.5, 4) == [2, 5, 1, 3]
    assert L.heavy_pixels(lane, 3.0, 100) == [2, 5, 1, 3, 7]            # strictly above the bar
    assert L.heavy_pixels(lane, 9.0, 100) == [] and L.heavy_pixels(lane, 0.0, 0) == []


def test_synthetic_cases_have_the_properties_the_gpu_test_relies_on(built):
    assert {c["n"] for c, _ in built.values()} == set(NS)
    seen = {k: set() for k in ("cap", "split", "cost", "rec_off", "xcd", "applied")}
    for name, (c, (order, mask, hpix, (total, cmax))) in built.items():
        n, kw = c["n"], c["kw"]
        assert sorted(order) == list(range(n)), name                    # a permutation
        assert total < 2 ** 53 and len(hpix) == min(c["n_cand"], kw["cap"], 64 * n), name
        assert sum(bin(m).count("1") for m in mask) == len(hpix), name
        steps, cost = L.tile_costs(c["records"].tolist(), kw["rec_off"], kw["learn_cost"])
        key = [min(x, L.KEY_MAX) for x in cost]
        seen["cost"].add(kw["learn_cost"]); seen["rec_off"].add(kw["rec_off"]); seen["xcd"].add(kw["xcd"])
        if kw["rec_off"]:
            assert (c["records"][:kw["rec_off"]] >= np.uint64(1 << 63)).all()   # junk the kernels must skip
        if c["kind"] == "ties" and n >= 8:
            shared = sum(1 for k in key if key.count(k) > 1)
            assert 4 * shared >= n, name                                # stability is exercised
            if kw["order_split"]:
                at = kw["order_split"] / 100.0 * float(max(key))
                assert any(float(k) == at for k in key) and any(float(k) < at for k in key), name
                seen["split"].add(kw["order_split"])
            lens = [int(c["lane"][q]) for q in hpix]
            assert len(lens) > len(set(lens)), name                     # the pixel-index tie-break decides
            seen["cap"].add("below" if kw["cap"] < c["n_cand"] else "equal" if kw["cap"] == c["n_cand"] else "above")
        if c["kind"] == "big" and n >= 8:
            assert max(cost) >= 2 ** 32 and order != list(range(n)), name
            assert kw["learn_cost"] == 0 or max(cost) > 2 ** 63, name   # the wrapped duration
            if kw["order_split"] == 100:
                assert cmax > L.KEY_MAX and key[order[0]] == L.KEY_MAX and order[0] != 0, name
        if c["kind"] == "zero":
            assert total == 0 and cmax == 0 and order == list(range(n)), name
        if c["kind"] == "none":
            assert c["n_cand"] == 0 and hpix == [] and not any(mask), name
        if c["kind"] == "all":
            assert c["n_cand"] == 64 * n, name
        if c["kind"] == "bar":
            old = scaled_bar(total, kw["heavy_pixel_factor"], kw["concurrent"], kw["resident"])
            heavy_old = {q for q in range(64 * n) if float(c["lane"][q]) > old}
            assert heavy_old != set(hpix) and total == kw_total(name), name
        if kw["xcd"]:
            applies = L.xcd_applies(n, kw["xcd"], kw["tiles_x"], kw["tiles_y"], kw["frames"])
            seen["applied"].add(applies)
            assert applies == (n % 8 == 0 and kw["tiles_x"] * kw["tiles_y"] * kw["frames"] == n), name
            plain = L.cost_order(cost, kw["order_split"])
            assert (order != plain) if applies and n > 8 else (order == plain or applies), name
    assert seen == {"cap": {"below", "equal", "above"}, "split": {20, 100}, "cost": {0, 1}, "rec_off": {0, 5},
                    "xcd": {0, 1, 2, 3}, "applied": {True, False}}


def kw_total(name):
    return int(name.rsplit("-t", 1)[1])


def brute_rank(n, band, tx, ty, frames):
    tiles = sorted(range(n), key=lambda t: (((t // tx) % ty // band) % 8, (t // tx) % ty, t // tx // ty, t % tx))
    rank = [0] * n
    for i, t in enumerate(tiles):
        rank[t] = i
    return rank


@pytest.mark.parametrize("tx,ty,frames", [(3, 16, 1), (2, 8, 4), (5, 48, 2), (1, 64, 1), (5, 50, 4), (10, 25, 4),
                                          (4, 250, 1), (8, 3, 3), (2, 1, 4), (8, 9, 1)])
@pytest.mark.parametrize("band", [1, 2, 3, 7, 4096])
def test_xcd_grouping_deals_the_eighths_of_the_ranking(tx, ty, frames, band):
    n = tx * ty * frames
    if n % 8:
        assert not L.xcd_applies(n, band, tx, ty, frames)
        return
    assert L.xcd_applies(n, band, tx, ty, frames) and not L.xcd_applies(n, 0, tx, ty, frames)
    rank = brute_rank(n, band, tx, ty, frames)
    assert L.xcd_rank(n, band, tx, ty, frames) == rank                  # partial last cycles of bands included
    rng = np.random.RandomState(n + band)
    plain = [int(t) for t in rng.permutation(n)]                        # any cost order
    got = L.xcd_group(plain, band, tx, ty, frames)
    assert sorted(got) == list(range(n))
    where = {t: i for i, t in enumerate(plain)}
    for c in range(8):
        mine = got[c::8]
        assert sorted(rank[t] for t in mine) == list(range(c * n // 8, (c + 1) * n // 8))
        assert [where[t] for t in mine] == sorted(where[t] for t in mine)      # the cost order survives within
        if ty % (8 * band) == 0:
            assert {((t // tx) % ty // band) % 8 for t in mine} == {c}         # one class of row bands per XCD


def test_learn_end_to_end_on_a_small_launch():
    """Worked by hand: 8 tiles in a 2 x 4 grid, xcd 1."""
    rec = [[0, 0, 0, 0, s, 0, 0, 0] for s in (4, 9, 9, 1, 0, 7, 9, 2)]
    lane = [0] * 512
    lane[5], lane[64 + 63], lane[70], lane[300] = 4, 9, 9, 2
    order, mask, hpix, (total, cmax) = L.learn(rec, lane, rec_off=0, learn_cost=0, order_split=0, heavy_pixel_factor=50,
                                               concurrent=2, resident=41, cap=3)
    assert (total, cmax) == (41, 9) and order == [1, 2, 6, 5, 0, 7, 3, 4]
    assert hpix == [70, 127, 5] and mask == [1 << 5, (1 << 6) | (1 << 63), 0, 0, 0, 0, 0, 0]   # bar 1.0: 2 > 1 but cap 3
    order = L.learn(rec, lane, rec_off=0, learn_cost=0, order_split=0, heavy_pixel_factor=50, concurrent=2,
                    resident=41, cap=3, xcd=1, tiles_x=2, tiles_y=4, frames=1)[0]
    assert order == list(range(8))                                      # one tile per eighth: rank order = raster here
