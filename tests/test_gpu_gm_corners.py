"""GPU parity: svt_hip_gm_detect_corners and svt_hip_gm_match_corners against the fixture of the reference's own
svt_av1_fast_corner_detect and svt_av1_determine_correspondence (tests/golden/gm_corners.npz), record for record.  Every plane, record and
the workspace of a test live in one guarded arena: a byte written outside the records and the workspace fails the test.  Every test makes
its calls twice, and both runs must give the fixture."""
import ctypes as C

import numpy as np
import pytest

import gm_cases as K
from arena import PATTERN, Arena, check_containment
from svtav1_hip import abi, device

pytestmark = pytest.mark.gpu
CORNERS_BYTES, MATCHES_BYTES = C.sizeof(abi.GmCorners), C.sizeof(abi.GmMatches)


class Uploaded:
    """Planes at ragged offsets, one corner record per plane, one match record per job and the workspace of one detect call over all the
    planes, in ONE device buffer; everything in between is a pattern that nobody may change."""

    def __init__(self, hip, planes, n_jobs=0):
        self.hip, self.planes = hip, list(planes)
        a, self.off = Arena(fill=PATTERN, tail=512), {}
        for i, n in enumerate(self.planes):
            self.off["plane", n] = a.add("plane " + n, K.plane_buf(n), skew=1 + 2 * i)
        base = a.add("corner records", nbytes=len(self.planes) * CORNERS_BYTES)     # d_out[i] of a detect call: consecutive records
        for i, n in enumerate(self.planes):
            self.off["corners", n] = base + i * CORNERS_BYTES
        self.outputs = [(base, len(self.planes) * CORNERS_BYTES)]
        if n_jobs:
            base = a.add("match records", nbytes=n_jobs * MATCHES_BYTES)
            self.outputs.append((base, n_jobs * MATCHES_BYTES))
        for j in range(n_jobs):
            self.off["matches", j] = base + j * MATCHES_BYTES
        self.ws_bytes = K.workspace_bytes(hip, self.planes)
        self.off["ws", 0] = a.add("workspace", nbytes=self.ws_bytes)
        self.outputs.append((self.off["ws", 0], self.ws_bytes))
        self.arena, self.before = a, a.build()
        self.buf = device.DeviceBuffer(hip, self.before.nbytes)
        self.buf.upload(self.before)

    def at(self, kind, which=0):
        return self.buf.ptr + self.off[kind, which]

    def detect(self, stream=None):
        """One call over all the planes"""
        arr = (abi.GmPlane * len(self.planes))(*[K.gm_plane(self.at("plane", n), K.PLANE[n]) for n in self.planes])
        return self.hip.svt_hip_gm_detect_corners(arr, len(self.planes), self.at("corners", self.planes[0]), self.at("ws"), self.ws_bytes, stream)

    def match(self, cases, stream=None):
        jobs = (abi.GmMatchJob * len(cases))(*[K.match_job(m, self.at("plane", m.frm), self.at("plane", m.ref), self.at("corners", m.frm),
                                                           self.at("corners", m.ref)) for m in cases])
        return self.hip.svt_hip_gm_match_corners(jobs, len(cases), self.at("matches", 0), stream)

    def image(self):
        return self.buf.download(np.uint8, (self.before.nbytes,))

    def corners(self, image, name):
        o = self.off["corners", name]
        return image[o:o + CORNERS_BYTES].view(abi.GM_CORNERS_DTYPE)[0]

    def matches(self, image, j):
        o = self.off["matches", j]
        return image[o:o + MATCHES_BYTES].view(abi.GM_MATCHES_DTYPE)[0]


def run(hip, rc, what):
    device.check(hip, rc, what)


def assert_corners(rec, name):
    count, found, xy = K.golden_corners(name)
    assert (int(rec["count"]), int(rec["found"])) == (count, found), name
    assert np.array_equal(rec["xy"][:2 * count].reshape(-1, 2), xy), name


def assert_matches(rec, case):
    want = K.golden_matches(case.name)
    assert int(rec["count"]) == len(want) and int(rec["pad_"]) == 0, case.name
    assert np.array_equal(rec["pts"][:4 * len(want)].reshape(-1, 4), want), case.name
    nf = K.used(K.golden_corners(case.frm)[0], case.frm_quarters)
    assert not rec["pts"][4 * len(want):4 * nf].any(), case.name      # the slots of the corners that gave none are cleared


@pytest.mark.parametrize("name", [p.name for p in K.PLANES])
def test_detection_equals_the_fixture(hip, name):
    u = Uploaded(hip, [name])
    for _ in range(2):
        run(hip, u.detect(), "svt_hip_gm_detect_corners")
        image = u.image()
        assert_corners(u.corners(image, name), name)
        check_containment(u.before, image, u.arena.regions, u.outputs, "svt_hip_gm_detect_corners " + name)
    rec = u.corners(image, name)
    count = int(rec["count"])       # nothing behind the last corner is written
    o = u.off["corners", name] + 8 + 8 * count
    assert np.array_equal(image[o:u.off["corners", name] + CORNERS_BYTES], u.before[o:u.off["corners", name] + CORNERS_BYTES])


def test_planes_of_three_sizes_in_one_call(hip):
    u = Uploaded(hip, K.DETECT_BATCH)
    for _ in range(2):
        run(hip, u.detect(), "svt_hip_gm_detect_corners")
        image = u.image()
        for n in K.DETECT_BATCH:
            assert_corners(u.corners(image, n), n)
        check_containment(u.before, image, u.arena.regions, u.outputs, "svt_hip_gm_detect_corners, three planes")


def test_eight_planes_in_one_call(hip):
    names = K.DETECT_LISTED
    assert len(names) == abi.GM_MAX_PLANES
    u = Uploaded(hip, names)
    for _ in range(2):
        run(hip, u.detect(), "svt_hip_gm_detect_corners")
        image = u.image()
        for n in names:
            assert_corners(u.corners(image, n), n)
        check_containment(u.before, image, u.arena.regions, u.outputs, "svt_hip_gm_detect_corners, eight planes")


@pytest.mark.parametrize("case", K.MATCHES, ids=lambda m: m.name)
def test_matching_equals_the_fixture(hip, case):
    """Detect and match on one stream with nothing in between: the match reads the records the detect call is still writing."""
    planes = list(dict.fromkeys([case.frm, case.ref]))
    u = Uploaded(hip, planes, 1)
    for _ in range(2):
        run(hip, u.detect(), "svt_hip_gm_detect_corners")
        run(hip, u.match([case]), "svt_hip_gm_match_corners")
        image = u.image()
        for n in planes:
            assert_corners(u.corners(image, n), n)
        assert_matches(u.matches(image, 0), case)
        check_containment(u.before, image, u.arena.regions, u.outputs, "svt_hip_gm_match_corners " + case.name)


def test_jobs_of_one_call_share_the_frames_record(hip):
    cases = [K.MATCH[n] for n in K.SHARED]
    planes = list(dict.fromkeys([c.frm for c in cases] + [c.ref for c in cases]))
    u = Uploaded(hip, planes, len(cases))
    for _ in range(2):
        run(hip, u.detect(), "svt_hip_gm_detect_corners")
        run(hip, u.match(cases), "svt_hip_gm_match_corners")
        image = u.image()
        for j, c in enumerate(cases):
            assert_matches(u.matches(image, j), c)
        check_containment(u.before, image, u.arena.regions, u.outputs, "svt_hip_gm_match_corners, shared records")


def test_empty_and_refused_calls_write_nothing(hip):
    case = K.MATCH["b2_sz7_q4"]
    u = Uploaded(hip, [case.frm, case.ref], 1)
    assert u.detect() == 0      # so that the records below are real ones
    arr = (abi.GmPlane * 1)(K.gm_plane(u.at("plane", case.frm), K.PLANE[case.frm]))
    before = u.image()
    assert hip.svt_hip_gm_detect_corners(arr, 0, u.at("corners", case.frm), u.at("ws"), u.ws_bytes, None) == 0
    assert hip.svt_hip_gm_detect_corners(arr, 1, u.at("corners", case.frm), u.at("ws"), 16, None) == K.BAD_PARAMETER
    assert b"svt_hip_gm_detect_corners" in hip.svt_hip_last_error()
    jobs = (abi.GmMatchJob * 1)(K.match_job(case._replace(match_sz=15), u.at("plane", case.frm), u.at("plane", case.ref), u.at("corners", case.frm),
                                            u.at("corners", case.ref)))
    assert hip.svt_hip_gm_match_corners(jobs, 0, u.at("matches", 0), None) == 0
    assert hip.svt_hip_gm_match_corners(jobs, 1, u.at("matches", 0), None) == K.BAD_PARAMETER
    assert b"svt_hip_gm_match_corners" in hip.svt_hip_last_error()
    run(hip, hip.svt_hip_stream_sync(None), "svt_hip_stream_sync")
    assert np.array_equal(u.image(), before)
