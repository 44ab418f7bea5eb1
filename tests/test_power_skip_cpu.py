"""CPU: what the fused binning pass (strided_c2c_kernel<R1, R2, 16, POWER = true>) leaves out, restated in numpy from the
kernel's thread geometry, loses no mode that FFTPower bins.

Geometry of one workgroup (k_y = batch index + ky0, tile of C = 16 columns from k_z0 = 16 * tile): thread (sub, c) holds
the rows k_x index sub + R1 * k2, k2 < R2; a wave is 64 / C = 4 consecutive `sub`.  Left out:

* the whole workgroup when k_y^2 + k_z0^2 > (N/2)^2 (forward pruning);
* the epilogue step (wave, k2) when (smallest |k_x| of the wave's four rows)^2 + k_y^2 + k_z0^2 > (N/2)^2;
* the column k_z = N/2 altogether: the k_y pass takes N/2 columns and the last pass counts the tile that starts there as
  pruned.  The one mode of that plane with |m| <= N/2, (0, 0, N/2), is dropped by both binning rules at these sides
  (last test).

A mode can be binned only if 0 < |m|^2 <= (N/2)^2: the integer rule takes |m| < N/2, the float64 rule may also let a vector
of norm exactly N/2 fall into the last shell.
"""
import numpy as np
import pytest

INSTANCES = {256: (16, 16, 16), 512: (16, 32, 16), 1024: (32, 32, 16)}        # N: (R1, R2, C) of dispatch_c2c<true>


def _box(i, n):
    return np.where(i > n // 2, i - n, i)


def wave_min_kx(n):
    """Per row index (k_x index sub + R1 * k2): the smallest |k_x| of the row's wave at that k2, as the kernel forms it."""
    R1, R2, C = INSTANCES[n]
    row = np.arange(n)
    sub, k2 = row % R1, row // R1
    per_wave = 64 // C
    wsub0 = sub // per_wave * per_wave
    wsub1 = wsub0 + per_wave - 1
    return np.where(R1 * k2 >= n // 2, n - (wsub1 + R1 * k2), wsub0 + R1 * k2)


def skipped_rows_by_tile(n, ky_index):
    """(pruned[tile], skipped[row, tile]) of the workgroups of global row k_y index `ky_index`, tiles of the N/2 columns."""
    R = n // 2
    ky = int(_box(np.int64(ky_index), n))
    kz0 = np.arange(R // 16) * 16
    pruned = ky * ky + kz0 * kz0 > R * R
    akx = wave_min_kx(n)
    skipped = akx[:, None] ** 2 + ky * ky + kz0[None, :] ** 2 > R * R
    return pruned, skipped | pruned[None, :]


def test_the_model_restates_the_wave_geometry():
    """wave_min_kx against a direct enumeration of the four rows of every wave."""
    for n, (R1, R2, C) in INSTANCES.items():
        assert R1 * R2 == n and C == 16 and (n // 2) % C == 0 and R1 % (64 // C) == 0
        akx = wave_min_kx(n)
        for k2 in range(R2):
            for w in range(R1 // 4):
                rows = np.arange(4 * w, 4 * w + 4) + R1 * k2
                assert (akx[rows] == np.abs(_box(rows, n)).min()).all(), (n, k2, w)


@pytest.mark.parametrize("n", [256, 512, 1024])
def test_no_binned_mode_lies_in_a_skipped_block_or_tile(n):
    R = n // 2
    kx = _box(np.arange(n), n).astype(np.int64)
    kz = np.arange(R, dtype=np.int64)
    kxz2 = kx[:, None] ** 2 + kz[None, :] ** 2
    nloc = n // 4                                       # slab blocks of a quarter of the rows: batch index b, offset ky0
    seen = 0
    for ky0 in range(0, n, nloc):
        for b in range(nloc):
            ky = int(_box(np.int64(b + ky0), n))
            norm2 = kxz2 + ky * ky
            binned = (norm2 > 0) & (norm2 <= R * R)                       # the edge |m| = N/2 included
            _, skipped = skipped_rows_by_tile(n, b + ky0)
            lost = binned & np.repeat(skipped, 16, axis=1)
            assert not lost.any(), (n, ky0, b, np.argwhere(lost)[:4])
            seen += int((binned & (norm2 == R * R)).sum())
    assert seen >= 2                                    # (N/2, 0, 0) and (0, N/2, 0) at least: the edge was looked at


@pytest.mark.parametrize("n", [256, 512, 1024])
def test_the_nyquist_column_holds_one_mode_that_can_be_binned(n):
    R = n // 2
    k = _box(np.arange(n), n).astype(np.int64)
    norm2 = k[:, None] ** 2 + k[None, :] ** 2 + R * R
    hit = np.argwhere(norm2 <= R * R)
    assert hit.tolist() == [[0, 0]]
    # and the oracle's float64 rule bins nothing of that plane, (0, 0, N/2) included, whatever the box
    from oracle import fftpower as offt
    for L in (1000.0, 100.0, 700.0):
        s = offt.shell_index(k, k, np.array([R], dtype=np.int64), norm2[:, :, None], n, L, "float64")
        assert not ((s >= 0) & (s < R - 1)).any(), (n, L)


@pytest.mark.parametrize("n", [256, 512, 1024])
def test_the_float64_rule_never_bins_the_nyquist_mode_of_a_power_of_two_side(n):
    """ast::float64_edge_norm(N/2, 0, 0, N/2, kf), restated: the mode falls into the last shell iff
    (kf N/2)^2 < (kf + (N/2 - 1) kf)^2 in doubles.  With N/2 = 2^k the left root is exact.  On the right, (2^k - 1) kf is
    rounded by at most half an ulp of kf 2^k (a quarter when it lies in the binade below); adding kf gives kf 2^k plus that
    error, which rounds back to kf 2^k - in the half-ulp tie kf's low k bits are 10...0, so kf 2^k has an even mantissa and
    wins the tie.  Both sides are the same double and `<` is false: power_3d_impl leaves the column out at every box size
    (it still asks the rule on the host and keeps the column if the answer were ever "binned")."""
    R = n // 2
    rng = np.random.default_rng(n)
    L = np.concatenate([np.arange(1.0, 4000.0, 0.25), rng.uniform(0.01, 1e5, 200000), np.exp(rng.uniform(-20, 20, 200000))])
    kf = 2.0 * np.pi / L
    kz = kf * float(R)
    k2 = (0.0 * kf + 0.0 * kf) + kz * kz
    e = kf + float(R - 1) * kf
    assert (e == kz).all()
    assert not (k2 < e * e).any()


def test_share_of_skipped_blocks_at_1024():
    """A third of the (wave, k2) steps of the workgroups that the pruning keeps hold no mode inside the sphere."""
    n = 1024
    R1, R2, _ = INSTANCES[n]
    total = skip = 0
    for kyi in range(n):
        pruned, skipped = skipped_rows_by_tile(n, kyi)
        blocks = skipped[:, ~pruned].reshape(R2, R1 // 4, 4, -1)          # rows -> (k2, wave, row of the wave)
        assert (blocks == blocks[:, :, :1]).all()                           # a wave's rows go together
        total += blocks[:, :, 0].size
        skip += int(blocks[:, :, 0].sum())
    share = skip / total
    print(f"skipped (wave, k2) blocks at N = 1024: {skip} of {total} = {share:.4f}")
    assert 0.30 <= share <= 0.35
