"""Restatement of E25, poses refined below a cell by Gauss-Newton on the bilinearly interpolated field
(include/rplgpu_msg.h, rplgpu_refine_poses_dev).  The sums have two writers: (a) Python integers, point by point, the
float32 front in numpy scalars; (b) vectorised numpy, int64 where a term fits and object (Python integer) arrays
where it does not.  The two must agree (tests/test_refine_cpu.py).  The step has two as well: the library's plain
C++ twin rplgpu_refine_step_host and the numpy.float64 restatement here.  Plus the spec check, the words' encoding,
the result words, the rounds chained, and the two joining rules.  TEST INFRASTRUCTURE — imported by tests/ only.

Points: tests/fused_oracle.group_points through tests/match_cases.case_points, the composition E8 - E15 use."""
from __future__ import annotations

import math

import numpy as np

from rplidar_ros2_driver_amd import abi

F32 = np.float32
F64 = np.float64
MAX_DIM = 4096
SCAN_CELL_RANGE = 0x2
WORDS = 32
STEPPED, FEW, SINGULAR, CLAMP_X, CLAMP_Y, CLAMP_T = 0x01, 0x02, 0x04, 0x08, 0x10, 0x20
QNAN = 0x7FC00000
DEFAULT = dict(origin_x=-25.6, origin_y=-25.6, resolution=0.05, width=1024, height=1024, target=127, damping=0.0,
               max_step_cells=2.0, max_rot=0.1, min_points=16)
# name -> (first word, limbs, signed): the header's table
LAYOUT = dict(sxx=(0, 2, False), sxy=(2, 2, True), syy=(4, 2, False), sxe=(6, 2, True), sye=(8, 2, True),
              sv=(10, 2, False), sxt=(12, 3, True), syt=(15, 3, True), stt=(18, 3, False), ste=(21, 3, True),
              see=(24, 3, False), n=(27, 1, False), dropped=(28, 1, False))


def spec(**kw) -> dict:
    d = dict(DEFAULT)
    for k in kw:
        if k not in d:
            raise KeyError(k)
    d.update(kw)
    return d


def struct_of(s: dict) -> "abi.PoseRefine":
    return abi.PoseRefine(s["origin_x"], s["origin_y"], s["resolution"], s["width"], s["height"], s["target"],
                          s["damping"], s["max_step_cells"], s["max_rot"], s["min_points"])


def spec_valid(s: dict) -> bool:
    f = [F32(s[k]) for k in ("origin_x", "origin_y", "resolution", "damping", "max_step_cells", "max_rot")]
    if not all(np.isfinite(v) for v in f):
        return False
    if not f[2] > 0 or not f[3] >= 0 or not f[4] > 0 or not f[5] > 0:
        return False
    if not (1 <= s["width"] <= MAX_DIM and 1 <= s["height"] <= MAX_DIM):
        return False
    return 1 <= s["target"] <= 127 and s["min_points"] >= 3


def scratch_words(G: int, P: int) -> int:
    return 0 if G == 0 or P == 0 or P > (1 << 20) else 2 * 29 * G * P


def finite_points(x, y):
    x, y = np.asarray(x, F32), np.asarray(y, F32)
    m = np.isfinite(x) & np.isfinite(y)
    return x[m], y[m]


def field_values(field) -> np.ndarray:
    return np.maximum(np.asarray(field, np.int8).astype(np.int64), 0)


# ---- the words -----------------------------------------------------------------------------------------------------
def to_words(sums: dict) -> np.ndarray:
    w = np.zeros(WORDS, np.uint32)
    for name, (at, limbs, signed) in LAYOUT.items():
        v = int(sums[name])
        bits = 32 * limbs
        assert (-(1 << (bits - 1)) <= v < (1 << (bits - 1))) if signed else (0 <= v < (1 << bits)), (name, v)
        v &= (1 << bits) - 1
        for i in range(limbs):
            w[at + i] = (v >> (32 * i)) & 0xFFFFFFFF
    return w


def from_words(w) -> dict:
    out = {}
    for name, (at, limbs, signed) in LAYOUT.items():
        v = sum(int(w[at + i]) << (32 * i) for i in range(limbs))
        if signed and v >> (32 * limbs - 1):
            v -= 1 << (32 * limbs)
        out[name] = v
    return out


# ---- writer (a): Python integers, point by point ------------------------------------------------------------------------
def sums_python(x, y, pose, s, field) -> dict:
    W, H = int(s["width"]), int(s["height"])
    f = field_values(field).reshape(H, W)
    c, sn, tx, ty = (F32(v) for v in pose)
    ox, oy, res = F32(s["origin_x"]), F32(s["origin_y"]), F32(s["resolution"])
    target = int(s["target"]) * 65536
    acc = {k: 0 for k in LAYOUT}

    def m(ix, iy):
        return int(f[iy, ix]) if 0 <= ix < W and 0 <= iy < H else 0

    with np.errstate(all="ignore"):
        for px, py in zip(np.asarray(x, F32), np.asarray(y, F32)):
            ax = F32(F32(c * px) - F32(sn * py))
            ay = F32(F32(sn * px) + F32(c * py))
            rx, ry = F32(ax + tx), F32(ay + ty)
            hu = F32(F32(F32(F32(rx - ox) / res) * F32(256)) - F32(128))
            hv = F32(F32(F32(F32(ry - oy) / res) * F32(256)) - F32(128))
            lx, ly = F32(ax / res), F32(ay / res)
            if not (abs(hu) < 2 ** 28 and abs(hv) < 2 ** 28 and abs(lx) < 8192 and abs(ly) < 8192):
                acc["dropped"] += 1
                continue
            U, V_ = int(math.floor(hu)), int(math.floor(hv))
            i0, a, j0, b = U >> 8, U & 255, V_ >> 8, V_ & 255
            Lx, Ly = int(np.rint(F32(lx * F32(16)))), int(np.rint(F32(ly * F32(16))))
            m00, m10, m01, m11 = m(i0, j0), m(i0 + 1, j0), m(i0, j0 + 1), m(i0 + 1, j0 + 1)
            V = (256 - a) * (256 - b) * m00 + a * (256 - b) * m10 + (256 - a) * b * m01 + a * b * m11
            Gx = (256 - b) * (m10 - m00) + b * (m11 - m01)
            Gy = (256 - a) * (m01 - m00) + a * (m11 - m10)
            Gt = Gy * Lx - Gx * Ly
            E = target - V
            for k, v in (("sxx", Gx * Gx), ("sxy", Gx * Gy), ("syy", Gy * Gy), ("sxe", Gx * E), ("sye", Gy * E),
                         ("sv", V), ("sxt", Gx * Gt), ("syt", Gy * Gt), ("stt", Gt * Gt), ("ste", Gt * E),
                         ("see", E * E), ("n", 1)):
                acc[k] += v
    return acc


# ---- writer (b): vectorised --------------------------------------------------------------------------------------------
def front(x, y, pose, s):
    """(kept mask, U, V_, Lx, Ly of the kept points) by the float32 front, vectorised."""
    x, y = np.asarray(x, F32), np.asarray(y, F32)
    c, sn, tx, ty = (F32(v) for v in pose)
    ox, oy, res = F32(s["origin_x"]), F32(s["origin_y"]), F32(s["resolution"])
    with np.errstate(all="ignore"):
        ax = ((c * x).astype(F32) - (sn * y).astype(F32)).astype(F32)
        ay = ((sn * x).astype(F32) + (c * y).astype(F32)).astype(F32)
        rx, ry = (ax + tx).astype(F32), (ay + ty).astype(F32)
        hu = ((((rx - ox).astype(F32) / res).astype(F32) * F32(256)).astype(F32) - F32(128)).astype(F32)
        hv = ((((ry - oy).astype(F32) / res).astype(F32) * F32(256)).astype(F32) - F32(128)).astype(F32)
        lx, ly = (ax / res).astype(F32), (ay / res).astype(F32)
        keep = (np.abs(hu) < F32(2 ** 28)) & (np.abs(hv) < F32(2 ** 28)) & (np.abs(lx) < F32(8192)) & \
               (np.abs(ly) < F32(8192))
        U = np.floor(hu[keep]).astype(np.int64)
        V_ = np.floor(hv[keep]).astype(np.int64)
        Lx = np.rint((lx[keep] * F32(16)).astype(F32)).astype(np.int64)
        Ly = np.rint((ly[keep] * F32(16)).astype(F32)).astype(np.int64)
    return keep, U, V_, Lx, Ly


def terms(x, y, pose, s, field):
    """(kept mask, dict of int64 arrays V, Gx, Gy, Gt, E, a, b, i0, j0, Lx, Ly over the kept points)."""
    W, H = int(s["width"]), int(s["height"])
    f = np.zeros((H + 2, W + 2), np.int64)  # a border of zeros: everything outside reads 0
    f[1:-1, 1:-1] = field_values(field).reshape(H, W)
    keep, U, V_, Lx, Ly = front(x, y, pose, s)
    i0, a, j0, b = U >> 8, U & 255, V_ >> 8, V_ & 255

    def m(ix, iy):
        return f[np.clip(iy + 1, 0, H + 1), np.clip(ix + 1, 0, W + 1)]

    m00, m10, m01, m11 = m(i0, j0), m(i0 + 1, j0), m(i0, j0 + 1), m(i0 + 1, j0 + 1)
    V = (256 - a) * (256 - b) * m00 + a * (256 - b) * m10 + (256 - a) * b * m01 + a * b * m11
    Gx = (256 - b) * (m10 - m00) + b * (m11 - m01)
    Gy = (256 - a) * (m01 - m00) + a * (m11 - m10)
    Gt = Gy * Lx - Gx * Ly
    E = int(s["target"]) * 65536 - V
    return keep, dict(V=V, Gx=Gx, Gy=Gy, Gt=Gt, E=E, a=a, b=b, i0=i0, j0=j0, Lx=Lx, Ly=Ly)


def sums_numpy(x, y, pose, s, field) -> dict:
    keep, t = terms(x, y, pose, s, field)
    Gx, Gy, E, V = t["Gx"], t["Gy"], t["E"], t["V"]
    Gt = t["Gt"].astype(object)  # Python integers: Gt^2 passes 2^64
    Eo, Gxo, Gyo = E.astype(object), Gx.astype(object), Gy.astype(object)
    tot = lambda a: int(a.sum()) if len(a) else 0  # noqa: E731
    return dict(sxx=tot(Gx * Gx), sxy=tot(Gx * Gy), syy=tot(Gy * Gy), sxe=tot(Gx * E), sye=tot(Gy * E), sv=tot(V),
                sxt=tot(Gxo * Gt), syt=tot(Gyo * Gt), stt=tot(Gt * Gt), ste=tot(Gt * Eo), see=tot(Eo * Eo),
                n=int(keep.sum()), dropped=int((~keep).sum()))


# ---- a group's sums ---------------------------------------------------------------------------------------------------
def sums_of(x, y, poses, s, field, writer=sums_numpy):
    """(sums (P, 32) uint32, result (8,) uint32 with words 0 - 3 zero, status without the truncated bit) of a
    group's points; poses that are equal bit for bit are computed once."""
    fx, fy = finite_points(x, y)
    poses = np.ascontiguousarray(poses, F32).reshape(-1, 4)
    uniq, inv = np.unique(poses.view(np.uint32), axis=0, return_inverse=True)
    got = np.stack([to_words(writer(fx, fy, u.view(F32), s, field)) for u in uniq])
    sums = got[inv.reshape(-1)]
    sv = [int(w[10]) | (int(w[11]) << 32) for w in sums]
    best = max(sv)
    q = sv.index(best)
    result = np.array([0, 0, 0, 0, q, best & 0xFFFFFFFF, best >> 32, len(fx)], np.uint64).astype(np.uint32)
    status = SCAN_CELL_RANGE if (sums[:, 28] != 0).any() else 0
    return sums, result, status


# ---- the step -----------------------------------------------------------------------------------------------------------
def _canon(v: np.float32) -> np.uint32:
    return np.uint32(QNAN) if np.isnan(v) else np.float32(v).view(np.uint32)


def step_numpy(words, s, pose):
    """(pose_out (4,) uint32 bits, step (4,) uint32) by the header's sequence in numpy.float64."""
    d = from_words(words)
    pose = np.asarray(pose, F32)
    flags = 0
    dx = dy = dt = F64(0)
    with np.errstate(all="ignore"):
        if d["n"] < s["min_points"]:
            flags = FEW
        else:
            def d64(v):
                return F64(float(v))  # Python's int -> float is the correctly rounded conversion

            def d96(name):
                at = LAYOUT[name][0]
                w0, w1, w2 = int(words[at]), int(words[at + 1]), int(words[at + 2])
                if LAYOUT[name][2] and w2 >> 31:
                    w2 -= 1 << 32
                return (F64(w2) * F64(2.0 ** 32) + F64(w1)) * F64(2.0 ** 32) + F64(w0)

            a11, a12, a22 = d64(d["sxx"]) * F64(2.0 ** -16), d64(d["sxy"]) * F64(2.0 ** -16), d64(d["syy"]) * F64(2.0 ** -16)
            a13, a23, a33 = d96("sxt") * F64(2.0 ** -20), d96("syt") * F64(2.0 ** -20), d96("stt") * F64(2.0 ** -24)
            g1, g2, g3 = d64(d["sxe"]) * F64(2.0 ** -24), d64(d["sye"]) * F64(2.0 ** -24), d96("ste") * F64(2.0 ** -28)
            damping = F64(F32(s["damping"]))
            a11 = a11 + damping * a11
            a22 = a22 + damping * a22
            a33 = a33 + damping * a33
            c11 = a22 * a33 - a23 * a23
            c12 = a13 * a23 - a12 * a33
            c13 = a12 * a23 - a13 * a22
            c22 = a11 * a33 - a13 * a13
            c23 = a12 * a13 - a11 * a23
            c33 = a11 * a22 - a12 * a12
            det = (a11 * c11 + a12 * c12) + a13 * c13
            if not (det > 0) or not np.isfinite(det):
                flags = SINGULAR
            else:
                dx = ((c11 * g1 + c12 * g2) + c13 * g3) / det
                dy = ((c12 * g1 + c22 * g2) + c23 * g3) / det
                dt = ((c13 * g1 + c23 * g2) + c33 * g3) / det
                flags = STEPPED if np.isfinite(dx) and np.isfinite(dy) and np.isfinite(dt) else SINGULAR
        out = pose.view(np.uint32).copy()
        mx = my = mt = F32(0)
        if flags & STEPPED:
            ms, mr = F64(F32(s["max_step_cells"])), F64(F32(s["max_rot"]))
            if dx > ms:
                dx, flags = ms, flags | CLAMP_X
            if dx < -ms:
                dx, flags = -ms, flags | CLAMP_X
            if dy > ms:
                dy, flags = ms, flags | CLAMP_Y
            if dy < -ms:
                dy, flags = -ms, flags | CLAMP_Y
            if dt > mr:
                dt, flags = mr, flags | CLAMP_T
            if dt < -mr:
                dt, flags = -mr, flags | CLAMP_T
            h = F64(0.5) * dt
            hh = h * h
            den = F64(1) + hh
            dc = (F64(1) - hh) / den
            ds = (h + h) / den
            fc, fs = F32(dc), F32(ds)
            res = F64(F32(s["resolution"]))
            mx, my, mt = F32(dx * res), F32(dy * res), F32(dt)
            c, sn, tx, ty = pose
            out = np.array([_canon(F32(F32(c * fc) - F32(sn * fs))), _canon(F32(F32(sn * fc) + F32(c * fs))),
                            _canon(F32(tx + mx)), _canon(F32(ty + my))], np.uint32)
    step = np.array([F32(mx).view(np.uint32), F32(my).view(np.uint32), F32(mt).view(np.uint32), flags], np.uint32)
    return out, step


def step_host(words, s, pose):
    """The same through the library's plain C++ twin."""
    out, step = abi.refine_step_host(np.asarray(words, np.uint32), struct_of(s), np.asarray(pose, F32))
    return out.view(np.uint32).copy(), step


def step_list(sums, s, poses, stepper=step_numpy):
    """(poses_out (P, 4) float32, step (P, 4) uint32, the four counts) of a group's list; equal (sums, pose) pairs
    are computed once."""
    poses = np.ascontiguousarray(poses, F32).reshape(-1, 4)
    key = np.concatenate([np.asarray(sums, np.uint32), poses.view(np.uint32)], 1)
    uniq, inv = np.unique(key, axis=0, return_inverse=True)
    got = [stepper(u[:WORDS], s, u[WORDS:].view(F32)) for u in uniq]
    out = np.stack([g[0] for g in got])[inv.reshape(-1)]
    step = np.stack([g[1] for g in got])[inv.reshape(-1)]
    fl = step[:, 3]
    counts = [int((fl & STEPPED != 0).sum()), int((fl & FEW != 0).sum()), int((fl & SINGULAR != 0).sum()),
              int((fl & (CLAMP_X | CLAMP_Y | CLAMP_T) != 0).sum())]
    return out.view(F32), step, counts


def refine_points(x, y, poses, s, field, iters=1, writer=sums_numpy, stepper=step_numpy):
    """`iters` rounds on a group's points: (poses_out (P, 4) float32, sums, step, result, status) as the device
    leaves them: the last round's sums, step words and result, every round's status."""
    poses = np.ascontiguousarray(poses, F32).reshape(-1, 4)
    status = 0
    for _ in range(iters):
        sums, result, st = sums_of(x, y, poses, s, field, writer)
        status |= st
        out, step, counts = step_list(sums, s, poses, stepper)
        result = result.copy()
        result[:4] = counts
        poses = out
    return poses, sums, step, result, status


# ---- the joints -------------------------------------------------------------------------------------------------------------
def match_pose(best, rot, K, res, pivot=None, prior=None) -> np.ndarray:
    """rplgpu_match_poses_dev for one group: (4,) float32.  rot: (2K + 1, 2) float32, the rotation table."""
    px, py = (F32(0), F32(0)) if pivot is None else (F32(pivot[0]), F32(pivot[1]))
    p0 = np.array([1, 0, px, py], F32) if prior is None else np.asarray(prior, F32).copy()
    k, j, i = (int(v) - (1 << 32) if int(v) >> 31 else int(v) for v in np.asarray(best, np.uint32)[1:4])
    if not -K <= k <= K:
        return p0
    c, s = F32(rot[k + K][0]), F32(rot[k + K][1])
    c0, s0, x0, y0 = p0
    res = F32(res)
    with np.errstate(all="ignore"):
        qx, qy = F32(x0 - px), F32(y0 - py)
        return np.array([F32(F32(c * c0) - F32(s * s0)), F32(F32(s * c0) + F32(c * s0)),
                         F32(F32(F32(F32(c * qx) - F32(s * qy)) + px) + F32(F32(i) * res)),
                         F32(F32(F32(F32(s * qx) + F32(c * qy)) + py) + F32(F32(j) * res))], F32)


def compose_pose(pose, mount=None) -> np.ndarray:
    """rplgpu_compose_poses_dev for one scan: the six floats of the composed pose."""
    c, s, x, y = (F32(v) for v in pose)
    r00, r01, tx, r10, r11, ty = (F32(v) for v in (mount if mount is not None else (1, 0, 0, 0, 1, 0)))
    with np.errstate(all="ignore"):
        return np.array([F32(F32(c * r00) - F32(s * r10)), F32(F32(c * r01) - F32(s * r11)),
                         F32(F32(F32(c * tx) - F32(s * ty)) + x),
                         F32(F32(s * r00) + F32(c * r10)), F32(F32(s * r01) + F32(c * r11)),
                         F32(F32(F32(s * tx) + F32(c * ty)) + y)], F32)
