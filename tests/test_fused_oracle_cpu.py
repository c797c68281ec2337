"""tests/fused_oracle.py without a GPU: the regime conditions of every input tests/test_gpu_fused_ror.py
runs (evaluated with the oracle alone), and the spec itself against what it must agree with — the C
oracle's own pipeline, a second writer (oracle/ext_second_writer.py: cKDTree ROR, np.unique grid), the
order of the scans, and the library's host merge of oracle-made cell records."""
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "oracle"))

from rplidar_ros2_driver_amd import Params, abi, synth  # noqa: E402
from tests import fused_oracle as fz  # noqa: E402
from tests import oracle_lib  # noqa: E402

XYZ_TOL = 1e-6
N = fz.N_FULL


# ---- the regime conditions (B) -----------------------------------------------------------------------------
@pytest.mark.parametrize("q_min", fz.Q_MINS)
def test_settled_regime(oracle, q_min):
    p = Params.defaults(**{**fz.P_C5, "q_min": q_min})
    batch, removed, late = fz.settled_batch(fz.SETTLED_SEED, fz.SETTLED_B, N)
    kept = fz.scans_kept(oracle, batch, p)
    for b in range(len(batch)):
        fz.settled_regime(batch[b], removed[b], late[b], kept[b], p)


@pytest.mark.parametrize("q_min", fz.Q_MINS)
def test_radius_regime(oracle, q_min):
    p = Params.defaults(**{**fz.P_C5, "q_min": q_min})
    batch, targets = fz.radius_batch(oracle, fz.RADIUS_SEED, N, p)
    assert any(t["exact"] for t in targets) and not all(t["exact"] for t in targets)
    for b, t in enumerate(targets):
        lo, hi = np.float32(t["r_lo"]), np.float32(t["r_hi"])
        assert np.nextafter(lo, np.float32(1.0)) == hi  # one ulp of ror_radius apart
        assert abs(float(hi) - 0.1) < 0.02
        kept = [fz.scan_kept(oracle, batch[b], Params.defaults(**{**fz.P_C5, "q_min": q_min, "ror_radius": float(r)}))
                for r in (lo, hi)]
        fz.radius_regime(kept[0], kept[1], t)


@pytest.mark.parametrize("q_min", fz.Q_MINS)
def test_redone_regime(oracle, q_min):
    p = Params.defaults(**{**fz.P_TIGHT, "q_min": q_min})
    for kept in fz.scans_kept(oracle, fz.redone_batch(fz.REDONE_SEED, fz.REDONE_B, N), p):
        fz.redone_regime(kept)


@pytest.mark.parametrize("pp", [fz.P_C5, fz.P_TIGHT], ids=["c5", "tight"])
def test_mixed_regime(oracle, pp):
    p = Params.defaults(**pp)
    batch, lens = fz.mixed_batch(fz.MIXED_SEED, N)
    assert lens[3] == 0 and {int(v) % fz.BLOCK for v in lens} >= {0, 1, fz.BLOCK - 1}
    fz.mixed_regime(fz.scans_kept(oracle, [batch[b, :lens[b]] for b in range(len(batch))], p), lens, p)


@pytest.mark.parametrize("clip", [0, 1])
@pytest.mark.parametrize("kind", fz.RANGE_KINDS)
def test_cell_range_regime(oracle, kind, clip):
    p = Params.defaults(**fz.range_params(clip))
    s = fz.range_scan(kind)
    out = fz.range_regime(kind, fz.scan_kept(oracle, s, p), p)
    _, _, _, status = fz.fused_grid(oracle, [s], p)
    assert status == (abi.SCAN_CELL_RANGE if out else 0)


def test_bench_c5_data_has_next_to_no_removals(oracle):
    """Why the bench's own C5 batch cannot show that E5 works: the oracle removes next to nothing from it (17
    of 3 704 505 kept points in its first 128 scans, at most 3 in a scan, none in nine scans of ten) — isolated
    singles only, never a survivor that the window or the whole-scan count has to put back."""
    p = Params.defaults(**fz.P_C5)
    kept = fz.scans_kept(oracle, synth.make_batch(2026 + 5, 16, N, noise_m=0.01), p)
    removed = [int((~k).sum()) for _, _, k in kept]
    assert max(removed) <= 3 and sum(removed) <= 1e-5 * sum(len(k) for _, _, k in kept), removed


# ---- the spec against its neighbours (D) --------------------------------------------------------------------
def _small_group(seed, n=4000, S=8):
    """Kinds 1, 3 and 4 at a size the second writer and the quadratic oracle finish quickly."""
    scans = []
    for s in range(S):
        if s % 3 == 0:
            scans.append(fz.settled_scan(seed, s, n)[0])
        elif s % 3 == 1:
            scans.append(synth.make_scan(seed + 1, s, n, noise_m=0.01, r0_range=(1.0, 4.0)))
        else:
            scans.append(fz.cluttered_scan(seed, s, n - 7 * s, count=6))
    scans[5] = fz.lonely_scan(seed, 5, n)
    scans[7] = scans[7][:0]
    return scans


def _xf(S, seed, n):
    rng = np.random.default_rng(seed)
    motion = np.stack([[rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(-0.3, 0.3), 0.1 / n]
                       for _ in range(S)]).astype(np.float32)
    ang = rng.uniform(-3, 3, S)
    pose = np.stack([np.cos(ang), -np.sin(ang), rng.uniform(-2, 2, S), np.sin(ang), np.cos(ang),
                     rng.uniform(-2, 2, S)], 1).astype(np.float32)
    t0 = rng.uniform(-0.05, 0.0, S).astype(np.float32)
    return motion, pose, t0


@pytest.mark.parametrize("pp", [fz.P_C5, {**fz.P_C5, "ror_radius": 0.03, "ror_min_neighbors": 3}], ids=["c5", "tight"])
def test_group_of_one_equals_cloud_pipeline(oracle, pp):
    p = Params.defaults(**pp)
    for s in _small_group(51) + [fz.settled_scan(52, 0, 24000)[0]]:
        want, wcells, wcounts = oracle.cloud_pipeline(s, oracle_lib.copy_params(p))
        got, cells, counts, status = fz.fused_grid(oracle, [s], p)
        assert status == 0
        assert got.tobytes() == want.tobytes() and np.array_equal(cells, wcells) and np.array_equal(counts, wcounts)


def test_scan_order_does_not_matter(oracle):
    p = Params.defaults(**fz.P_C5)
    scans = _small_group(53)
    motion, pose, t0 = _xf(len(scans), 5, 4000)
    kept = fz.scans_kept(oracle, scans, p)
    a = fz.fused_grid(oracle, scans, p, motion, pose, t0, kept=kept)
    order = [5, 2, 7, 0, 6, 1, 4, 3]
    b = fz.fused_grid(oracle, [scans[i] for i in order], p, motion[order], pose[order], t0[order],
                      kept=[kept[i] for i in order])
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3] == b[3] == 0
    assert np.max(np.abs(a[0][:, :2].astype(np.float64) - b[0][:, :2])) <= XYZ_TOL
    assert np.array_equal(a[0][:, 2], b[0][:, 2])


@pytest.mark.parametrize("pp", [fz.P_C5, {**fz.P_C5, "ror_radius": 0.03, "ror_min_neighbors": 3}], ids=["c5", "tight"])
def test_second_writer_agrees_on_the_group_grid(oracle, pp):
    """E1, E2, E5 and E4 by oracle/ext_second_writer.py, E6 and the pose by fusion_oracle (the only
    statement of them): ROR decisions, cells, counts and intensity bits equal, centroids within 1e-6 m."""
    import ext_second_writer as w2
    import fusion_oracle as fo
    p = Params.defaults(**pp)
    scans = _small_group(54)
    motion, pose, t0 = _xf(len(scans), 6, 4000)
    kept = fz.scans_kept(oracle, scans, p)
    pts = []
    for s, nodes in enumerate(scans):
        kw = dict(is_new_protocol=bool(p.is_new_protocol), inverted=bool(p.inverted), clip_enable=bool(p.clip_enable),
                  q_min=p.q_min, range_min=p.range_min, range_max=p.range_max)
        cloud = w2.scan_to_points(nodes, **kw)
        idx = np.flatnonzero(w2.keep_mask(nodes, clip_enable=bool(p.clip_enable), q_min=p.q_min,
                                          range_min=p.range_min, range_max=p.range_max))
        k = w2.ror_keep(cloud, p.ror_radius, p.ror_min_neighbors)
        assert np.array_equal(idx, kept[s][1]) and np.array_equal(k, kept[s][2]), s
        cloud = fo.deskew_cloud(cloud[k], idx[k], motion[s], t0[s])
        r00, r01, tx, r10, r11, ty = pose[s]
        pts.append(fo.transform_cloud(cloud, np.array([[r00, r01, 0, tx], [r10, r11, 0, ty], [0, 0, 1, 0]], np.float32)))
    assert sum(int((~k).sum()) for _, _, k in kept) > 0
    want, wcells, wcounts = w2.voxel_grid(np.concatenate(pts), p.voxel_leaf)
    got, cells, counts, status = fz.fused_grid(oracle, scans, p, motion, pose, t0, kept=kept)
    assert status == 0 and np.array_equal(cells, wcells) and np.array_equal(counts, wcounts)
    assert got[:, 3].tobytes() == want[:, 3].tobytes()
    assert np.max(np.abs(got[:, :2].astype(np.float64) - want[:, :2])) <= XYZ_TOL


@pytest.mark.parametrize("split", [[[0, 1, 2, 3], [4, 5, 6, 7]], [[s] for s in range(8)], [[5, 0, 7], [2, 6], [1, 4, 3]]])
def test_host_merge_of_oracle_records_equals_fused_grid(oracle, split):
    """tests/test_cells_cpu.py with E5 removing points: records written from the oracle's points of every
    rank's sensors, merged by rplgpu_merge_cells_host, are the fused grid bit for bit (points with |x|, |y| >=
    3.125 cm, where the record sums are exact)."""
    from tests.test_cells_cpu import cells_of, rank_slot
    p = Params.defaults(**fz.P_C5)
    groups = [_small_group(55), _small_group(56)]
    per_group = []
    for g, scans in enumerate(groups):
        motion, pose, t0 = _xf(len(scans), 7 + g, 4000)
        kept = fz.scans_kept(oracle, scans, p)
        assert sum(int((~k).sum()) for _, _, k in kept) > 0
        pts, slot = fz.group_cloud_points(oracle, scans, p, motion, pose, t0, kept=kept)
        big = (np.abs(pts[:, 0]) >= 0.03125) & (np.abs(pts[:, 1]) >= 0.03125)
        per_group.append((pts[big], slot[big]))
    per_rank = [[cells_of(pts[np.isin(slot, sensors)]) for pts, slot in per_group] for sensors in split]
    slot_cells = max(sum(len(c) for c in r) for r in per_rank) + 5
    slots, metas = zip(*(rank_slot(r, slot_cells, 2) for r in per_rank))
    arena, cursor, starts, npts, status = abi.merge_cells_host(np.stack(slots), slot_cells, np.stack(metas),
                                                               len(split), 2, p)
    total = 0
    for g, (pts, _) in enumerate(per_group):
        want, _, _ = oracle.voxel_grid(pts, p.voxel_leaf)
        assert int(npts[g]) == len(want) and status[g] == 0
        assert arena[int(starts[g]): int(starts[g]) + int(npts[g])].tobytes() == want.tobytes()
        total += len(want)
    assert cursor == total
