"""GridIndexTable (ct_nbr_table_*, ct_nbr_radius_multi): one launch over centres of mixed clouds returns, bit for bit, the
rows the per-cloud GridIndex.query_radius returns — three clouds of 1, 700 and 20 000 points, whose grids differ in
origin, cell edge and dims."""
import numpy as np
import pytest
import torch

from tests.test_nbr_gpu import area_like

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def setup():
    from cloud_transformers_amd.neighbors import GridIndex, GridIndexTable
    rng = np.random.default_rng(5)
    clouds = [np.float32([[1.0, 2.0, 3.0]]),
              rng.uniform(-1.0, 1.0, (700, 3)).astype(np.float32) * np.float32([1.5, 1.0, 0.5]),
              area_like(20000, 9, size=(9.0, 6.0, 3.0))]
    indices = [GridIndex(torch.from_numpy(p).cuda()) for p in clouds]
    assert len({tuple(ix.dims) for ix in indices}) == 3 and len({ix.h for ix in indices}) == 3
    table = GridIndexTable(indices)
    assert table.offsets == [0, 1, 701] and table.max_points == 20000
    cloud = [2, 0, 1, 2, 1, 0, 2]                                            # mixed, repeated, not sorted
    centres = np.float32([clouds[2][17],                                       # a point of the big cloud
                          [1.0, 2.0, 3.0],                                      # the single point itself: count 1 < K
                          [0.2, -0.1, 0.0],                                     # inside the 700: count 700 at r = 2
                          [500.0, -500.0, 500.0],                               # far outside every box: count 0
                          [9.0, 9.0, 9.0],                                      # outside the 700's box
                          [1.1, 2.1, 3.0],                                      # near the single point
                          clouds[2][4321] + np.float32([0.01, -0.02, 0.005])])
    return indices, table, torch.tensor(cloud, device="cuda"), torch.from_numpy(centres).cuda()


@pytest.mark.parametrize("r", [0.3, 2.0])
@pytest.mark.parametrize("K", [1, 64, 2048])
def test_table_query_equals_per_cloud_queries(setup, K, r):
    indices, table, cloud, centres = setup
    idx, d2, count = table.query_radius(cloud, centres, r, K)
    assert idx.shape == (7, K) and idx.dtype == torch.int64 and d2.dtype == torch.float32 and count.dtype == torch.int64
    host_cloud = cloud.tolist()
    for q, c in enumerate(host_cloud):
        wi, wd, wc = indices[c].query_radius(centres[q:q + 1], r, K)
        assert torch.equal(count[q:q + 1], wc), (q, c)
        assert torch.equal(idx[q], wi[0]), (q, c)
        assert torch.equal(d2[q].view(torch.int32), wd[0].view(torch.int32)), (q, c)
    got = count.tolist()
    assert got[3] == 0 and int(idx[3].max()) == -1                            # nothing in reach: -1 / +inf throughout
    assert got[1] == 1 and (K == 1 or int(idx[1, 1]) == -1)                    # fewer than K in the ball
    if r == 2.0:
        assert got[2] == 700 and got[0] > 64
    assert min(got[0], got[6]) > 1


def test_table_refuses_bad_input(setup):
    from cloud_transformers_amd.neighbors import GridIndexTable
    indices, table, cloud, centres = setup
    with pytest.raises(ValueError):
        GridIndexTable([])
    with pytest.raises(ValueError):
        GridIndexTable(indices, offsets=[0, 1])
    with pytest.raises(ValueError):
        table.query_radius(cloud[:3], centres, 1.0, 8)                          # one cloud id per centre
    with pytest.raises(ValueError):
        table.query_radius(cloud.int(), centres, 1.0, 8)
    with pytest.raises(RuntimeError):
        table.query_radius(cloud.cpu(), centres, 1.0, 8)                        # no CPU path
    assert table.query_radius(cloud[:0], centres[:0], 1.0, 8)[0].shape == (0, 8)
