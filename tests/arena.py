"""One host image of a device buffer for every GPU test, and one check that a kernel wrote nothing outside its declared outputs
(test infrastructure)."""
import numpy as np

GUARD = 0xA5            # the byte of guard runs, stride padding and result buffers that nobody may write
PATTERN = "pattern"     # Arena(fill=PATTERN): byte i starts as pattern(i), so that a byte copied from elsewhere shows as well


def pattern(size):
    return ((np.arange(size, dtype=np.uint32) * 37 + 11) & 0xFF).astype(np.uint8)


class Arena:
    """Host image of one device buffer: arrays at aligned offsets, each recorded as (offset, bytes, name) in `regions`.  fill is what
    every byte that no input array covers starts as, outputs included: a constant byte or PATTERN; tail: bytes behind the last array."""

    def __init__(self, fill=0, tail=0):
        self.fill, self.tail, self.chunks, self.regions, self.size = fill, tail, [], [], 0

    def add(self, name, arr=None, nbytes=None, align=256, gap=256, skew=0):
        """Offset of the array (or of an output of nbytes) `skew` bytes past the next multiple of `align`; what follows starts at least
        `gap` bytes behind its end."""
        off = -(-self.size // align) * align + skew
        nbytes = arr.nbytes if arr is not None else nbytes
        self.regions.append((off, nbytes, name))
        if arr is not None:
            self.chunks.append((off, np.ascontiguousarray(arr).view(np.uint8).reshape(-1)))
        self.size = -(-(off + nbytes) // align) * align + gap
        return off

    def build(self):
        size = self.size + self.tail
        buf = pattern(size) if self.fill == PATTERN else np.full(size, self.fill, np.uint8)
        for off, a in self.chunks:
            buf[off:off + a.size] = a
        return buf


def rows(off, stride, row_bytes, h):
    """The declared (offset, bytes) of a strided output: one entry per row (stride in bytes)."""
    return [(off + r * stride, row_bytes) for r in range(h)]


def check_containment(before, after, regions, declared, what=""):
    """Every byte that no (offset, bytes) of `declared` covers is what it was before the call."""
    free = np.ones(before.size, bool)
    for off, nb in declared:
        free[off:off + nb] = False
    bad = np.flatnonzero((after != before) & free)
    if bad.size:
        o, where = int(bad[0]), "before the first array"
        for off, nb, name in regions:
            if off <= o:
                where = name if o < off + nb else "slack after " + name
        raise AssertionError(f"{what}: byte {o} ({where}) changed from {before[o]} to {after[o]}; {bad.size} bytes in all")


class OnDevice:
    """Device copies of host buffers (blend_cases.Buf)."""

    def __init__(self, hip, bufs):
        from svtav1_hip import device
        self.bufs, self.ptrs = {}, {}
        for b in bufs:
            d = device.DeviceBuffer(hip, b.a.nbytes)
            d.upload(b.a)
            self.bufs[id(b)], self.ptrs[id(b)] = d, d.ptr

    def fetch(self, buf):
        """Overwrite the host buffer with its device copy."""
        buf.a[:] = self.bufs[id(buf)].download(buf.a.dtype, buf.a.shape)
