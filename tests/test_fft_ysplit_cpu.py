"""Host: the factorisation behind the y-split route of the fused fp32 power passes, restated in numpy.

N = 16 S.  The z pass takes rows y2 + S j (j < 16) of a plane, forms A[k1] = sum_j X_j w_16^(j k1), multiplies by
w_N^(y2 k1) and stores row k1 S + y2; the k_y pass transforms the S consecutive rows of block k1 in place, output k2 to
row k1 S + k2.  Row b of a plane then holds k_y = (b // S) + 16 (b mod S), and the pruning of both strided passes asks
the parent's rule of that index.
"""
import numpy as np
import pytest

SIDES = (256, 512, 1024)


def permuted_ky(n):
    """k_y held by row b of a plane, b < n."""
    s = n // 16
    b = np.arange(n)
    return (b // s) + 16 * (b % s)


def signed(k, n):
    return np.where(k > n // 2, k - n, k)


def disc_row_in(n, row, kz0):
    """The parent's rule (disc_row_in of fft_tile.hip with the tile's first column): the edge itself stays."""
    ky = row - n if row > n // 2 else row
    return ky * ky + kz0 * kz0 <= (n // 2) ** 2


def four_step(x):
    """The two passes on an (n, cols) array, rows = y: returns the permuted layout."""
    n = x.shape[0]
    s = n // 16
    w = np.exp(-2j * np.pi * np.arange(n) / n)
    z = np.empty_like(x)
    for y2 in range(s):                                   # z pass, workgroup y2: rows y2 + s j
        a = np.fft.fft(x[y2::s], axis=0)                  # A[k1] = sum_j X_j w_16^(j k1)
        for k1 in range(16):
            z[k1 * s + y2] = a[k1] * w[(y2 * k1) % n]
    out = np.empty_like(x)
    for k1 in range(16):                                  # k_y pass: s points over the block's consecutive rows
        out[k1 * s:(k1 + 1) * s] = np.fft.fft(z[k1 * s:(k1 + 1) * s], axis=0)
    return out


@pytest.mark.parametrize("n", SIDES)
def test_four_step_identity_with_the_layout_permutation(n):
    rng = np.random.default_rng(n)
    x = rng.standard_normal((n, 3)) + 1j * rng.standard_normal((n, 3))
    ref = np.fft.fft(x, axis=0)
    got = four_step(x)
    scale = np.abs(ref).max()
    err = np.abs(got - ref[permuted_ky(n)]).max() / scale
    print(f"n={n}: largest difference / largest value {err:.2e}")
    # both sides are float64 transforms of n points: a few n eps at most; a wrong twiddle or row is O(1)
    assert err <= 64 * n * 2.0 ** -53


@pytest.mark.parametrize("n", SIDES)
def test_permutation_is_a_bijection(n):
    ky = permuted_ky(n)
    assert sorted(ky.tolist()) == list(range(n))
    s, ysh = n // 16, (n // 16).bit_length() - 1
    b = np.arange(n)
    assert np.array_equal(ky, (b >> ysh) + ((b & (s - 1)) << 4))           # the kernel's shifts
    # block k1 holds k1 + 16 k2: what the k_y pass's store rule uses
    for k1 in (0, 1, 15):
        assert np.array_equal(ky[k1 * s:(k1 + 1) * s], k1 + 16 * np.arange(s))


@pytest.mark.parametrize("cols", [16, 32])
@pytest.mark.parametrize("n", SIDES)
def test_permuted_pruning_keeps_exactly_the_parents_rows(n, cols):
    """For every tile of 16 and of 32 columns: the rows b kept by signed(k1 + 16 k2)^2 + k_z0^2 <= (N/2)^2 hold exactly the
    k_y that the parent's rule keeps."""
    ky = permuted_ky(n)
    h2 = (n // 2) ** 2
    tiles = (n // 2 + 1 + cols - 1) // cols
    for tile in range(tiles):
        kz0 = cols * tile
        kept = signed(ky, n) ** 2 + kz0 * kz0 <= h2
        want = {row for row in range(n) if disc_row_in(n, row, kz0)}
        assert set(ky[kept].tolist()) == want, (n, cols, tile)
        assert kept.sum() == len(want)
    # the rule prunes something and keeps something at either tile width
    assert not all(disc_row_in(n, n // 2, cols * t) for t in range(tiles)) and disc_row_in(n, 0, cols * (tiles - 1))
