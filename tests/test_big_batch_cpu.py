"""The conditions that make tests/test_gpu_big_batch.py meaningful, evaluated with the oracles alone (no
device): the templates of tests/big_batch_cases.py exercise both filters, no two of them give the same
result, and the template a launch would read with one `+ b0` forgotten — 24 rows away in the second piece of
65535 scans, 48 in the third — is never the same as the right one.  Should a change of the generator miss a
condition, the generator is to be adjusted, not the condition."""
import numpy as np
import pytest

from tests import big_batch_cases as bb

CONFIGS = [(1, 1), (1, 0), (0, 1), (0, 0)]  # (scan_processing, circular)


def _rows(out, removed, counts):
    """Per template what the device writes: (count, the bits of the beams below count, both counts)."""
    bits = np.ascontiguousarray(out, np.float32).view(np.uint32)
    return [(int(c), bits[k, : int(c)].tobytes(), tuple(int(v) for v in removed[k])) for k, c in enumerate(counts)]


def test_the_moduli():
    assert bb.B == 2 * 65535 + 3 and bb.PIECE % bb.K == 24 and (2 * bb.PIECE) % bb.K == 48
    assert all(bb.K % d for d in range(2, bb.K))  # prime
    counts = bb.template_counts()
    assert sorted(set(counts.tolist())) == list(range(bb.N_STRIDE + 1))
    assert sorted(set(bb.template_point_counts().tolist())) == list(range(bb.MAX_POINTS + 1))


@pytest.mark.parametrize("sp,circular", CONFIGS)
def test_templates_exercise_both_filters_and_are_distinct(sp, circular):
    ranges, _ = bb.template_scans()
    counts = bb.template_counts()
    out, removed = bb.filter_templates(ranges, counts, sp, circular)
    assert (removed[:, 0] > 0).sum() >= 60, int((removed[:, 0] > 0).sum())
    assert (removed[:, 1] > 0).sum() >= 60, int((removed[:, 1] > 0).sum())
    rows = _rows(out, removed, counts)
    assert len(set(rows)) == bb.K
    for k in range(bb.K):
        assert rows[k] != rows[(k + 24) % bb.K] and rows[k] != rows[(k + 48) % bb.K], k
    # a scan keeps beams, so that a wrong template shows in the ranges and not in the intensities alone
    kept = np.isfinite(np.where(np.arange(bb.N_STRIDE)[None, :] < counts[:, None], out, np.nan)).sum(1)
    assert (kept[counts >= 3] > 0).all()


@pytest.mark.parametrize("circular", [1, 0])
def test_merged_templates(circular):
    ranges, _ = bb.template_scans()
    out, removed = bb.filter_merged_templates(ranges, circular)
    assert (removed[:, 0] > 0).sum() >= 60 and (removed[:, 1] > 0).sum() >= 60
    rows = _rows(out, removed, np.full(bb.K, bb.MERGED_COUNT))
    assert len(set(rows)) == bb.K
    for k in range(bb.K):
        assert rows[k] != rows[(k + 24) % bb.K] and rows[k] != rows[(k + 48) % bb.K], k


def test_inputs_differ_24_and_48_rows_apart():
    """The stages that only move data (messages, transform): counts or contents differ."""
    ranges, inten = bb.template_scans()
    pts, npts, counts = bb.template_clouds(), bb.template_point_counts(), bb.template_counts()
    for k in range(bb.K):
        for d in (24, 48):
            j = (k + d) % bb.K
            assert npts[k] != npts[j]
            c = int(min(counts[k], counts[j]))
            assert counts[k] != counts[j] or ranges[k, :c].tobytes() != ranges[j, :c].tobytes()
            assert counts[k] != counts[j] or inten[k, :c].tobytes() != inten[j, :c].tobytes()
    assert len({pts[k].tobytes() for k in range(bb.K)}) == bb.K
    # stamps, durations and poses come from b and are different for every scan
    assert len(np.unique(bb.stamps()[:, 0])) == bb.B and len(np.unique(bb.durations())) == bb.B
    d = bb.durations()
    assert np.array_equal(d.astype(np.float32).astype(np.float64), d)
    pose = bb.poses(bb.scan_template_index())
    assert np.array_equal(pose[:, 3].astype(np.float64), np.arange(bb.B))


def test_transform_restatement_against_fp64():
    """The float32 restatement of rpl_fuse.hip stays within a few ulp of the fp64 product (it is the
    reference of the device test, so it is held to something itself)."""
    kidx = bb.scan_template_index()[:: 997]
    pts = bb.template_clouds()[kidx]
    pose = bb.poses(bb.scan_template_index())[:: 997]
    got = bb.transform_points(pts, pose).astype(np.float64)
    m = pose.astype(np.float64).reshape(-1, 3, 4)
    want = np.einsum("brc,bpc->bpr", m[:, :, :3], pts[..., :3].astype(np.float64)) + m[:, None, :, 3]
    # three roundings of sums of terms bounded by |R| * 30 + |t|
    scale = np.abs(m[:, :, :3]).sum(2)[:, None, :] * 30.0 + np.abs(m[:, None, :, 3])
    assert np.max(np.abs(got[..., :3] - want) / scale) <= 4 * 2.0 ** -24
    assert got[..., 3].astype(np.float32).tobytes() == pts[..., 3].tobytes()
