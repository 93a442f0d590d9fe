"""CPU: tests/arena.py places arrays where the builders it replaced placed them, and its containment check names a stray byte wherever it
falls, one that holds a value found elsewhere in the image included."""
import numpy as np
import pytest

from arena import GUARD, PATTERN, Arena, check_containment, pattern, rows


class OldArena:
    """The builder tx_cases.Arena was, kept to compare with: 256-byte aligned offsets, 256 bytes of slack, zeros elsewhere"""

    def __init__(self):
        self.chunks, self.size = [], 0

    def add(self, arr=None, nbytes=None):
        off = self.size
        nbytes = arr.nbytes if arr is not None else nbytes
        self.chunks.append((off, None if arr is None else np.ascontiguousarray(arr).view(np.uint8).reshape(-1)))
        self.size += (nbytes + 255) // 256 * 256 + 256
        return off

    def build(self):
        buf = np.zeros(self.size, np.uint8)
        for off, a in self.chunks:
            if a is not None:
                buf[off:off + a.size] = a
        return buf


def test_defaults_reproduce_the_old_builder():
    rng = np.random.default_rng(1)
    arrays = [rng.integers(1, 256, n, dtype=np.uint8) for n in (1, 255, 256, 257)] + [rng.integers(1, 1 << 15, (3, 43)).astype(np.int16)]
    old, new = OldArena(), Arena()
    for k, a in enumerate(arrays):
        assert new.add(f"array {k}", a) == old.add(a)
        if k == 2:
            assert new.add("output", nbytes=100) == old.add(nbytes=100)
    assert np.array_equal(new.build(), old.build())
    assert new.regions[3] == (3 * 512, 100, "output") and len(new.regions) == 6


def test_align_and_skew_reproduce_the_packed_builders():
    """intra_pred_cases.Arena was: at = round_up(at, align) + lead; place; at += bytes.  subpel_cases.Arena the same with 64 and a shift."""
    for align, skew in ((16, 3), (64, 1)):
        ab, at = Arena(fill=GUARD, tail=64), 0
        for k, n in enumerate((1, 17, 64, 5, 130)):
            lead = skew if k % 2 else 0
            at = -(-at // align) * align + lead
            assert ab.add(f"array {k}", np.full(n, k, np.uint8), align=align, gap=0, skew=lead) == at
            at += n
        img = ab.build()
        assert img.size >= at + 64 and (img[ab.regions[1][0] - skew:ab.regions[1][0]] == GUARD).all() and (img[-64:] == GUARD).all()


def test_fills():
    for fill, want in ((0, np.zeros(1024, np.uint8)), (GUARD, np.full(1024, GUARD, np.uint8)), (PATTERN, pattern(1024))):
        ab = Arena(fill=fill)
        off = ab.add("input", np.arange(10, dtype=np.uint8))
        ab.add("output", nbytes=10)
        want = want.copy()
        want[off:off + 10] = np.arange(10)
        assert np.array_equal(ab.build(), want), fill
    assert np.array_equal(pattern(300), [(37 * i + 11) & 0xFF for i in range(300)])


@pytest.fixture(scope="module")
def layout():
    """An input 7 bytes into the image (the bytes in front of it belong to nobody), a skewed output, and an output of 4 rows of 6 bytes
    at a pitch of 10"""
    ab = Arena(fill=PATTERN)
    first = ab.add("input", np.arange(40, dtype=np.uint8), skew=7)
    skewed = ab.add("skewed output", nbytes=30, skew=12)
    strided = ab.add("strided output", nbytes=4 * 10)
    return ab.build(), ab.regions, first, skewed, strided, [(skewed, 30)] + rows(strided, 10, 6, 4)


@pytest.mark.parametrize("where, name", [("before", "before the first array"), ("gap", "slack after input"), ("skew slack", "slack after skewed output"),
                                         ("stride padding", "strided output")])
def test_a_stray_byte_is_named(layout, where, name):
    before, regions, first, skewed, strided, declared = layout
    at = {"before": first - 1, "gap": first + 40 + 3, "skew slack": skewed + 30, "stride padding": strided + 10 + 7}[where]
    after = before.copy()
    after[at] ^= 0x40
    with pytest.raises(AssertionError, match=rf"byte {at} \({name}\) changed from {before[at]} to {after[at]}; 1 bytes in all"):
        check_containment(before, after, regions, declared, "case")


def test_declared_bytes_may_change(layout):
    before, regions, _, _, _, declared = layout
    after = before.copy()
    for off, nb in declared:
        after[off:off + nb] ^= 0xFF
    check_containment(before, after, regions, declared)
    check_containment(before, before.copy(), regions, [])


def test_a_copied_neighbour_is_seen(layout):
    """A byte that takes the value its neighbour holds: a constant fill cannot tell, the pattern can."""
    before, regions, _, skewed, _, declared = layout
    at = skewed + 30 + 5
    after = before.copy()
    after[at] = before[at + 1]
    assert after[at] != before[at]
    with pytest.raises(AssertionError, match=rf"byte {at} \(slack after skewed output\)"):
        check_containment(before, after, regions, declared)
    const = np.full(before.size, GUARD, np.uint8)
    same = const.copy()
    same[at] = const[at + 1]
    check_containment(const, same, regions, declared)       # what the constant fill misses
