"""The heavy-first learning (DESIGN.md "heavy-first", csrc/rt_learn.hip and
rt_runtime.hip learn_order) as a model in plain Python: what a learning
launch's per-tile records and per-pixel walk lengths become.  Integers
throughout; floats only where the contract is a double computation (the
order_split threshold and the heavy-pixel bar), written in the host path's
order of operations.  Python's float is the C double, its int -> float
conversion and its division are correctly rounded as C's are.

    learn(records, lane, ...) -> order[n], mask[n], hpix[<= cap], (total, cmax)
"""
KEY_MAX = 2 ** 32 - 1          # a tile's sort key saturates here: costlier tiles tie
U64 = 2 ** 64


def tile_costs(records, rec_off, learn_cost):
    """(steps, cost) per tile.  Tile k's record is records[rec_off + k] (a fused
    launch in an order writes its heavy-pixel waves' records first): words 0-1
    its wave's start and end ticks, 4 its lockstep steps, 5 its cooperative
    windows.  steps = w4 + 2 w5 always; the cost is the steps (learn_cost 0)
    or the duration w1 - w0 in 64-bit unsigned arithmetic (learn_cost 1)."""
    steps, cost = [], []
    for r in records[rec_off:]:
        s = (int(r[4]) + 2 * int(r[5])) % U64
        steps.append(s)
        cost.append(s if learn_cost == 0 else (int(r[1]) - int(r[0])) % U64)
    return steps, cost


def cost_order(cost, order_split):
    """Tiles at or above order_split percent of the costliest go first, most
    expensive first, ties in raster order; the rest keep raster order.
    order_split 0: every tile by cost.  Costs are compared as their keys
    (saturated at KEY_MAX), the threshold in double as the host writes it."""
    key = [min(c, KEY_MAX) for c in cost]
    split_at = float(order_split) / 100.0 * float(max(key, default=0))
    first = [k for k in range(len(key)) if order_split == 0 or float(key[k]) >= split_at]
    lead = set(first)
    first.sort(key=lambda k: -key[k])                   # stable
    return first + [k for k in range(len(key)) if k not in lead]


def heavy_bar(total, heavy_pixel_factor, concurrent, resident):
    """The host's px_bar: heavy_pixel_factor percent of the bulk estimate, the
    launch's total steps counted `concurrent` times and spread over the
    resident waves.  Three double roundings: the product, the quotient, and
    the final product (factor / 100.0 is a fourth, of a constant)."""
    t = float(total) * float(max(1, concurrent))
    bulk = t / float(max(1, resident))
    return heavy_pixel_factor / 100.0 * bulk


def heavy_pixels(lane, bar, cap):
    """Pixels whose walk length exceeds the bar, longest first, then the lower
    pixel index, at most cap of them."""
    cand = [q for q in range(len(lane)) if float(int(lane[q])) > bar]
    cand.sort(key=lambda q: (-int(lane[q]), q))
    return cand[:max(0, cap)]


def xcd_applies(n, xcd, tiles_x, tiles_y, frames):
    """The grouping needs whole eighths and the launch's tile grid."""
    return xcd > 0 and n % 8 == 0 and tiles_x > 0 and tiles_y > 0 and frames > 0 and tiles_x * tiles_y * frames == n


def xcd_rank(n, band, tiles_x, tiles_y, frames):
    """rank[t] of tile t = (frame * tiles_y + row) * tiles_x + column in the
    order of (row class, row, frame, column), a row's class being
    (row / band) % 8."""
    place, rows = {}, 0                                  # a row's place among the rows in class order
    for c in range(8):
        for row in range(tiles_y):
            if (row // band) % 8 == c:
                place[row] = rows
                rows += 1
    rank = [0] * n
    for t in range(n):
        col, by = t % tiles_x, t // tiles_x
        f, row = by // tiles_y, by % tiles_y
        rank[t] = (place[row] * frames + f) * tiles_x + col
    return rank


def xcd_group(order, band, tiles_x, tiles_y, frames):
    """Workgroups are dealt to the 8 XCDs round-robin, so position j of the
    order runs on XCD j % 8.  Eighth c holds the tiles of ranks
    [c n/8, (c+1) n/8), in the cost order; position r * 8 + c takes its r-th."""
    n = len(order)
    m = n // 8
    rank = xcd_rank(n, band, tiles_x, tiles_y, frames)
    eighth = [[t for t in order if rank[t] // m == c] for c in range(8)]
    out = [0] * n
    for c in range(8):
        for r, t in enumerate(eighth[c]):
            out[r * 8 + c] = t
    return out


def learn(records, lane, *, rec_off, learn_cost, order_split, heavy_pixel_factor, concurrent, resident, cap,
          xcd=0, tiles_x=0, tiles_y=0, frames=0):
    """records: rec_off + n rows of 8 words; lane: 64 n walk lengths.  Returns
    (order, mask, hpix, (total, cmax)): the launch order of the n tiles, every
    tile's 64-bit mask of its heavy pixels, the heavy pixels (tile * 64 + lane)
    and the launch's total steps and costliest cost (unsaturated)."""
    n = len(records) - rec_off
    assert n >= 1 and len(lane) == 64 * n
    steps, cost = tile_costs(records, rec_off, learn_cost)
    order = cost_order(cost, order_split)
    if xcd_applies(n, xcd, tiles_x, tiles_y, frames):
        order = xcd_group(order, xcd, tiles_x, tiles_y, frames)
    total = sum(steps)
    hpix = heavy_pixels(lane, heavy_bar(total, heavy_pixel_factor, concurrent, resident), min(max(cap, 0), 64 * n))
    mask = [0] * n
    for q in hpix:
        mask[q >> 6] |= 1 << (q & 63)
    return order, mask, hpix, (total, max(cost))
