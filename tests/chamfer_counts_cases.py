"""Helpers of the Chamfer-with-counts tests: lattice clouds with poisoned padding rows, the per-cloud oracle results, and the
forward case the metric tests reuse (built once per process)."""
import functools

import torch

from oracle import ref_cpu as R

FWD_CASE = (4, 300, 1003, [300, 0, 1, 129], [1003, 17, 0, 7])


def poison(x, counts, copies):
    """Fill rows [counts[b], n) of x [B,n,3] in place: copies of that cloud's own valid rows where `copies[b]` and it has
    any (a kernel that ignores the counts then reports distance 0 at an index at or beyond the count), NaN elsewhere."""
    B, n, _ = x.shape
    for b in range(B):
        c = int(counts[b])
        if c >= n:
            continue
        if copies[b] and c > 0:
            x[b, c:] = x[b, torch.arange(n - c) % c]
        else:
            x[b, c:] = float("nan")
    return x


def lattice_clouds(B, n, m, cnt1, cnt2, seed):
    """randint(0, 6) / 4 coordinates (every distance exact, ties abundant); padding poisoned: copies in clouds 2, 3 mod 4,
    NaN in clouds 0, 1 mod 4."""
    g = torch.Generator().manual_seed(seed)
    a = torch.randint(0, 6, (B, n, 3), generator=g).float() / 4
    b = torch.randint(0, 6, (B, m, 3), generator=g).float() / 4
    copies = [k % 4 >= 2 for k in range(B)]
    return poison(a, cnt1, copies), poison(b, cnt2, copies)


def oracle_with_counts(a, b, cnt1, cnt2):
    """oracle.ref_cpu.chamfer_fwd on each pair's own rows, laid out as ct_chamfer_fwd_counts lays its outputs out: dist 0 and
    idx -1 at the rows at or beyond a count and in every row of a cloud whose target cloud is empty."""
    B, n, m = a.shape[0], a.shape[1], b.shape[1]
    d1, d2 = torch.zeros(B, n), torch.zeros(B, m)
    i1, i2 = torch.full((B, n), -1, dtype=torch.int32), torch.full((B, m), -1, dtype=torch.int32)
    for k in range(B):
        c1, c2 = int(cnt1[k]), int(cnt2[k])
        if c1 == 0 or c2 == 0:
            continue
        r = R.chamfer_fwd(a[k:k + 1, :c1], b[k:k + 1, :c2])
        d1[k, :c1], d2[k, :c2], i1[k, :c1], i2[k, :c2] = r[0][0], r[1][0], r[2][0].int(), r[3][0].int()
    return d1, d2, i1, i2


@functools.lru_cache(maxsize=None)
def forward_case():
    """The forward case of the issue (B4 n300 m1003; an empty query cloud, an empty target cloud, fewer targets than the 16
    wave slices, a count that is no multiple of the 8-target block, a count just past a 128-query workgroup) ->
    (a, b, cnt1, cnt2 as lists, oracle outputs), all on the host and not to be modified."""
    B, n, m, cnt1, cnt2 = FWD_CASE
    a, b = lattice_clouds(B, n, m, cnt1, cnt2, seed=20)
    return a, b, cnt1, cnt2, oracle_with_counts(a, b, cnt1, cnt2)


def counts_tensor(counts, device="cuda"):
    return torch.tensor(list(counts), dtype=torch.int32, device=device)
