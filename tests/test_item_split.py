"""ItemMap::split (rip_device.hpp) restated in numpy float32 and compared with exact integer division over the domain the
library accepts.

The chain, statistics and vec4-remap kernels turn an item index into (row, 4-pixel group) with one float32 multiply by the
rounded reciprocal of the groups per row and one correction step.  The estimate is
    fl(fl(item) * fl(1 / g))  =  (item / g) (1 + e1)(1 + e2)(1 + e3),   |e_k| <= 2^-24,
so it lies within (item / g) * 3.0000004 * 2^-24 of the true quotient.  One correction step is enough while that stays below 1,
that is while item / g -- the row index -- stays below 2^24 / 3 = 5 592 405.  make_plan (rip_plan.cpp) accepts at most 2^22 =
4 194 304 rows, so the error is at most 0.75 everywhere in the domain; items stay below 2^32 / 12 < 2^31, so the int
arithmetic of the correction cannot wrap either.  The samples below are the rows where the estimate is worst (the largest
quotients) and the items where one step too few shows (the first and the last item of a row)."""
import numpy as np
import pytest

MAX_SIDE = 1 << 22
MAX_PIXELS = ((1 << 32) - 1) // 3           # rows * cols * 3 < 2^32 (rip_plan.cpp make_plan)


def max_rows(groups):
    """The largest row count the domain allows for rows of `groups` 4-pixel groups."""
    return min(MAX_SIDE, MAX_PIXELS // (4 * groups))


def split(items, groups):
    """ItemMap::split on an int64 array of items: (q, rem, steps) with steps the corrections applied (-1, 0, +1)."""
    inv = np.float32(1.0) / np.float32(groups)                       # ItemMap{g, 1.0f / (float)g}
    q = (items.astype(np.float32) * inv).astype(np.int64)            # (int)((float)item * inv_groups): truncation
    rem = items - q * groups
    lo, hi = rem < 0, rem >= groups
    q = q - lo + hi
    rem = rem + lo * groups - hi * groups
    return q, rem, hi.astype(np.int64) - lo.astype(np.int64)


def check_rows(groups, rows):
    """First, middle and last item of the given rows."""
    rows = np.asarray(rows, np.int64)
    for g_in_row in sorted({0, groups // 2, groups - 1}):
        items = rows * groups + g_in_row
        assert int(items.max()) < (1 << 31)
        q, rem, _ = split(items, groups)
        bad = np.flatnonzero((q != rows) | (rem != g_in_row))
        assert bad.size == 0, "groups %d: item %d splits into (%d, %d), exact (%d, %d); %d items wrong" % (
            groups, int(items[bad[0]]), int(q[bad[0]]), int(rem[bad[0]]), int(rows[bad[0]]), g_in_row, bad.size)


# every row for these; for the other small counts every 9th row and the last 65536 (the largest quotients)
DENSE_GROUPS = (1, 2, 3, 5, 8, 16, 33, 64, 85)


@pytest.mark.parametrize("groups", range(1, 86))
def test_small_group_counts_at_the_largest_row_count(groups):
    """Rows of 4 to 340 pixels: the frame can be 2^22 rows high (85 groups: floor(2^32 / 3 / 340) = 4 210 752 >= 2^22), so the
    quotient reaches its maximum over the whole domain here."""
    n = max_rows(groups)
    assert n == MAX_SIDE
    if groups in DENSE_GROUPS:
        rows = np.arange(n, dtype=np.int64)
    else:
        rows = np.unique(np.concatenate([np.arange(0, n, 9, dtype=np.int64), np.arange(n - 65536, n, dtype=np.int64)]))
    check_rows(groups, rows)


LARGE_GROUPS = sorted({g for k in range(7, 21) for g in ((1 << k) - 1, 1 << k, (1 << k) + 1) if g <= (1 << 20)} |
                      {86, 100, 341, 1000, 4099, 16381, 17500, 65535, 65537, 87381, 99991, 333333, 1000003, (1 << 20) - 3})


@pytest.mark.parametrize("groups", LARGE_GROUPS)
def test_larger_group_counts_up_to_the_widest_row(groups):
    """86 groups to 2^20 (a row of 2^22 pixels): the row count is what the 4 GiB limit leaves, every row is sampled."""
    assert groups <= (1 << 20)
    check_rows(groups, np.arange(max_rows(groups), dtype=np.int64))


def test_the_correction_step_is_needed_and_one_is_enough():
    """The estimate alone is wrong somewhere (the test above is not vacuous), and it is never further than one off."""
    seen = set()
    for groups in (1, 3, 85, 16383, 65535, 1 << 20):
        n = max_rows(groups)
        rows = np.arange(max(0, n - (1 << 18)), n, dtype=np.int64)
        for g_in_row in (0, groups - 1):
            items = rows * groups + g_in_row
            inv = np.float32(1.0) / np.float32(groups)
            est = items.astype(np.float32).astype(np.float64) * np.float64(inv)   # the product before its own rounding
            assert np.abs(est - items / groups).max() < 0.75
            seen.update(np.unique(split(items, groups)[2]).tolist())
    assert seen == {-1, 0, 1}, seen


def test_the_bound_of_the_domain_statement():
    """2^22 rows keep the error bound 3.0000004 * 2^-24 * rows below 1, and every accepted frame's items fit an int."""
    assert 3.0000004 * 2.0 ** -24 * MAX_SIDE <= 0.7500001
    assert MAX_SIDE < (1 << 24) // 3
    assert MAX_PIXELS // 4 + (1 << 20) < (1 << 31)   # (q + 1) * groups_per_row of the correction step
