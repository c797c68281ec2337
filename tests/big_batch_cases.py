"""Inputs of tests/test_gpu_big_batch.py: batches of B = 2 * 65535 + 3 tiny scans, so that the five launchers
which split a batch over gridDim.y in pieces of 65535 (rpl_filter.hip, rpl_msg.hip x 2, rpl_fuse.hip,
rpl_merge.hip) make three launches, the last of three scans, and offset every per-scan pointer twice.

Scan b is built from template row k = b % 251 (ranges, intensities, beam count, cloud points, point count)
and from b itself (stamp, scan duration, pose).  251 is prime and 65535 = 24 (mod 251): a launch that
forgot one `+ b0` reads, for the scans of the second piece, the template 24 rows away, and 48 rows away in
the third — tests/test_big_batch_cpu.py states that these always differ.  (257 and 17 divide 65535: with
them a forgotten offset would read the very same template.)

The oracles run on the 251 templates only; the B scans are compared against them vectorised."""
import math

import numpy as np

from tests import filter_oracle as fo

F32 = np.float32
PIECE = 65535            # gridDim.y limit: scans per launch
B = 2 * PIECE + 3        # 131073
K = 251                  # templates
N_STRIDE = 16            # beams per LaserScan slot
MERGED_COUNT = 12        # beams of a merged scan (rplgpu_filter_merged_scans_dev, the merged messages)
MAX_POINTS = 8           # points per cloud slot
FID = "laser_frame"
SENTINEL = F32(7.0)

# the filter settings of the issue: W = 2, N = 1, L = 3, everything else the defaults
FILTER = dict(shadow_window=2, shadow_neighbors=1, speckle_min_run=3)
# a merged scan of 12 beams over 5.4 rad: inc = 0.45, as a LaserScan of 14 beams (y = 1 lies below half a radian)
MERGE_SPEC = dict(angle_min=-2.7, angle_max=2.7, count=MERGED_COUNT, range_min=0.0, range_max=64.0,
                  scan_time=0.125)

# the b at which whole messages are compared with the CDR oracle: both ends of every piece
EDGE_B = (0, 1, PIECE - 1, PIECE, PIECE + 1, B - 4, B - 3, B - 2, B - 1)


def sample_b(seed=2026, n=2000):
    """EDGE_B and n seeded random scans."""
    rng = np.random.default_rng(seed)
    return np.unique(np.concatenate([np.asarray(EDGE_B), rng.integers(0, B, n)]))


def template_counts():
    """Beam count of template k: 0, 1 and 2 once each (with L = 3 a scan that short loses every finite
    beam, so two of them could not be told apart by their ranges), 3 .. 16 on the other even rows, and
    14 .. 16 on the odd rows — the shadow test looks only at pairs at most half a radian apart, which in
    Mode B (inc = 2 pi / (count - 1)) needs 14 beams."""
    k = np.arange(K)
    c = np.where(k % 2 == 1, 14 + (k // 2) % 3, 3 + (k // 2) % 14)
    c[0], c[2], c[4] = 0, 1, 2
    return c.astype(np.uint32)


def template_point_counts():
    """Points of template k's cloud: 0 .. 8; rows 24 and 48 apart differ (24 = 6, 48 = 3 mod 9; and across
    the wrap 24 - 251 = 7, 48 - 251 = 4 mod 9)."""
    return (np.arange(K) % (MAX_POINTS + 1)).astype(np.uint32)


def template_scans(seed=1):
    """(K, N_STRIDE) float32 ranges and intensities.  A row is a string of surfaces 1 .. 6 beams long at
    distances spread over 0.5 .. 40 m with +-1 cm of noise (beams of one surface link under the speckle
    rule's D = 5 cm; a near surface next to a far one makes the far edge a shadow pair; the first surface has
    at least L = 3 beams, so that a scan of 3 beams can keep them), and about one empty bin (+inf) in 16
    behind the first three beams."""
    rng = np.random.default_rng(seed)
    r = np.empty((K, N_STRIDE), F32)
    for k in range(K):
        row = []
        while len(row) < N_STRIDE:
            level = math.exp(rng.uniform(math.log(0.5), math.log(40.0)))
            row += [level + rng.uniform(-0.01, 0.01) for _ in range(int(rng.integers(1 if row else 3, 7)))]
        r[k] = np.asarray(row[:N_STRIDE], F32)
    r[:, 3:][rng.random((K, N_STRIDE - 3)) < 1.0 / 16.0] = np.inf
    inten = rng.integers(0, 64 * 4, r.shape).astype(F32) / F32(4.0)
    return r, inten


def template_clouds(seed=6):
    """(K, MAX_POINTS, 4) float32 points with every mantissa bit in use."""
    rng = np.random.default_rng(seed)
    return rng.uniform(-30.0, 30.0, (K, MAX_POINTS, 4)).astype(F32)


def scan_template_index():
    return (np.arange(B) % K).astype(np.int64)


def stamps():
    """(B, 2): sec = b (int32), nanosec = 7 * b (uint32), as the two words of rplgpu_stamp_t."""
    b = np.arange(B, dtype=np.int64)
    return np.stack([b, 7 * b], 1).astype(np.uint32)


def durations():
    """scan_duration of scan b: (b + 1) / 2^20 s — different for every b and exact in fp64 and float32."""
    return (np.arange(B, dtype=np.float64) + 1.0) / 2.0 ** 20


def poses(k_of_b):
    """(B, 12) float32 row-major [R | t]: a rotation about z by template-dependent angle with a shear term
    so that every coefficient matters, and the translation (b, -b, b / 2), exact in float32."""
    b = np.arange(B, dtype=np.float64)
    a = 0.05 * (k_of_b.astype(np.float64) + 1.0)
    m = np.zeros((B, 12), np.float64)
    m[:, 0], m[:, 1], m[:, 2], m[:, 3] = np.cos(a), -np.sin(a), 0.125, b
    m[:, 4], m[:, 5], m[:, 6], m[:, 7] = np.sin(a), np.cos(a), -0.25, -b
    m[:, 8], m[:, 9], m[:, 10], m[:, 11] = 0.0625, -0.03125, 1.0, 0.5 * b
    return m.astype(F32)


def transform_points(pts, pose):
    """rpl_fuse.hip restated: float32, products then sums left to right, one rounding each (numpy has no
    fused multiply-add); intensity untouched.  pts (B, P, 4), pose (B, 12) -> (B, P, 4)."""
    x, y, z = pts[..., 0], pts[..., 1], pts[..., 2]
    out = pts.copy()
    for row in range(3):
        r0, r1, r2, t = (pose[:, 4 * row + j][:, None] for j in range(4))
        acc = (r0 * x).astype(F32) + (r1 * y).astype(F32)
        acc = acc.astype(F32) + (r2 * z).astype(F32)
        out[..., row] = acc.astype(F32) + t
    return out


def filter_templates(ranges, counts, scan_processing, circular):
    """The E10 oracle on the templates: (K, N_STRIDE) output rows holding SENTINEL at and beyond the count
    (what a sentinel-filled output buffer keeps), and removed (K, 2)."""
    f = fo.flt(circular=circular, **FILTER)
    rows = np.where(np.arange(N_STRIDE)[None, :] < counts[:, None], ranges, SENTINEL).astype(F32)
    return fo.filter_batch(rows, counts, scan_processing, f)


def merged_inc():
    return F32((float(F32(MERGE_SPEC["angle_max"])) - float(F32(MERGE_SPEC["angle_min"]))) / MERGED_COUNT)


def filter_merged_templates(ranges, circular):
    """The E10 oracle on the first MERGED_COUNT beams of every template with the merged scan's increment."""
    f = fo.flt(circular=circular, **FILTER)
    out = np.empty((K, MERGED_COUNT), F32)
    removed = np.zeros((K, 2), np.int64)
    for k in range(K):
        out[k], removed[k, 0], removed[k, 1] = fo.filter_scan(ranges[k, :MERGED_COUNT], merged_inc(), f)
    return out, removed
