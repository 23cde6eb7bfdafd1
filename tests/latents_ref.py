"""NumPy restatement of the latent-set generator (csrc/latents.hip): Philox4x32-10, the gray-code Sobol sequence from
torch's own direction numbers, the two scrambles, the set composition and u.  Integer stage in uint32 / uint64 arrays, bit for bit what
the kernel computes; the value stage is left to the tests (torch.special.ndtri / ndtr in float64)."""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)
KINDS = {'sobol': 0, 'random': 1}
SCRAMBLES = {None: 0, 'shift': 1, 'owen': 2}
MOMENT_SEED = 20221                  # the moment tests' seed: tests/test_latents.py holds the restatement itself to their bounds at it


def philox4x32_10(c0, c1, c2, c3, key):
    """Ten Philox rounds on arrays of counter words (broadcast against each other); key: 64-bit int.  Returns four uint32 arrays."""
    c = [np.asarray(v, dtype=np.uint64) & M32 for v in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = np.uint64(key & 0xFFFFFFFF), np.uint64((key >> 32) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & M32]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return [v.astype(np.uint32) for v in c]


def philox_words(agents, zdim, word3, key):
    """[len(agents), len(word3), zdim] uint32: Philox(key, [a_lo, a_hi, d >> 2, word3])[d & 3]."""
    a = np.asarray(agents, dtype=np.uint64)[:, None, None]
    w3 = np.asarray(word3, dtype=np.uint64)[None, :, None]
    q = np.arange((zdim + 3) // 4, dtype=np.uint64)[None, None, :]
    out = philox4x32_10(a & M32, a >> np.uint64(32), q, w3, key)
    return np.stack(out, axis=-1).reshape(a.shape[0], w3.shape[1], -1)[:, :, :zdim]


def directions(zdim):
    """[zdim, 30] uint32: the 30-bit direction numbers of torch's SobolEngine."""
    import torch
    st = torch.quasirandom.SobolEngine(zdim).sobolstate.numpy()
    assert st.shape == (zdim, 30) and st.min() >= 0 and st.max() < (1 << 30)
    return st.astype(np.uint32)


def sobol_ints(P, zdim):
    """[P, zdim] uint32: x of point j = XOR over the set bits b of gray(j) of dirs[d, b] << 2."""
    dirs = directions(zdim) << np.uint32(2)
    j = np.arange(P, dtype=np.uint32)
    g = j ^ (j >> np.uint32(1))
    x = np.zeros((P, zdim), np.uint32)
    for b in range(max(1, int(P - 1).bit_length())):
        x ^= np.where(((g >> np.uint32(b)) & np.uint32(1))[:, None] == 1, dirs[None, :, b], np.uint32(0))
    return x


def brev(x):
    x = np.asarray(x, dtype=np.uint32)
    x = ((x >> np.uint32(1)) & np.uint32(0x55555555)) | ((x & np.uint32(0x55555555)) << np.uint32(1))
    x = ((x >> np.uint32(2)) & np.uint32(0x33333333)) | ((x & np.uint32(0x33333333)) << np.uint32(2))
    x = ((x >> np.uint32(4)) & np.uint32(0x0F0F0F0F)) | ((x & np.uint32(0x0F0F0F0F)) << np.uint32(4))
    x = ((x >> np.uint32(8)) & np.uint32(0x00FF00FF)) | ((x & np.uint32(0x00FF00FF)) << np.uint32(8))
    return (x >> np.uint32(16)) | (x << np.uint32(16))


def lk_hash(x, s):
    """Laine-Karras hash in Burley's form on 32-bit wrap-around arithmetic."""
    x = (np.asarray(x, dtype=np.uint64) + np.asarray(s, dtype=np.uint64)) & M32
    for m in (0x6c50b47c, 0xb82f1e52, 0xc7afe638, 0x8d22f6e6):
        x ^= (x * np.uint64(m)) & M32
    return x.astype(np.uint32)


def point_ints(n, P, zdim, kind='sobol', scramble='owen', seed=0, first_agent=0):
    """[n, P, zdim] uint32: the integer x of drawn point j < P of agents first_agent .. first_agent + n - 1."""
    agents = first_agent + np.arange(n, dtype=np.uint64)
    if KINDS[kind] == 1:
        return philox_words(agents, zdim, 1 + np.arange(P), seed)
    x = np.broadcast_to(sobol_ints(P, zdim)[None], (n, P, zdim))
    mode = SCRAMBLES[scramble]
    if mode == 0:
        return x.copy()
    s = philox_words(agents, zdim, [0], seed)                      # [n, 1, zdim]
    return x ^ s if mode == 1 else brev(lk_hash(brev(x), s))


def drawn_points(M, antithetic=False, center=False):
    """(c, H, B): the centre offset, the number of drawn points and of non-centre set members."""
    c = int(bool(center))
    B = M - c
    return c, ((B + 1) // 2 if antithetic else B), B


def set_ints(n, K, R, zdim, antithetic=False, center=False, **kw):
    """([n, M, zdim] uint32 bits, [n, M] int8 sign): per set index the integer behind it (0 where none is drawn) and +1 drawn / -1
    mirrored (its value is minus that of index m - H) / 0 centre."""
    M = R * K
    c, H, B = drawn_points(M, antithetic, center)
    bits = np.zeros((n, M, zdim), np.uint32)
    bits[:, c:c + H] = point_ints(n, H, zdim, **kw)
    sign = np.zeros((n, M), np.int8)
    sign[:, c:c + H] = 1
    sign[:, c + H:] = -1
    return bits, sign


def to_rounds(x, K):
    """[n, M, ...] set-index view -> the generator's layout [R, n K, ...] (set index m at round m // K, column m % K)."""
    n, M = x.shape[:2]
    R = M // K
    return np.ascontiguousarray(np.moveaxis(x.reshape(n, R, K, *x.shape[2:]), 1, 0)).reshape(R, n * K, *x.shape[2:])


def from_rounds(z, n, K):
    """The inverse of to_rounds for an array [R, n K, ...]."""
    R = z.shape[0]
    return np.ascontiguousarray(np.moveaxis(z.reshape(R, n, K, *z.shape[2:]), 0, 1)).reshape(n, R * K, *z.shape[2:])


def uniforms(bits):
    """u = (x + 0.5) 2^-32 in float64 (exact)."""
    return (np.asarray(bits).astype(np.uint32).astype(np.float64) + 0.5) * 2.0 ** -32


def quantiles(bits, truncate=None):
    """float64 z behind the integers, from torch's own ndtri / ndtr on the CPU: ndtri(u), or for truncate = t the quantile of
    u' = ndtr(-t) + u (ndtr(t) - ndtr(-t)), clipped to +-float32(t).

    u' is written as 0.5 + q with q = (u - 0.5) w, w = ndtr(t) - ndtr(-t): the same number (ndtr(-t) + w / 2 = 0.5), but q carries the
    digits of a value near the mode, which the sum next to ndtr(-t) rounds to a multiple of 2^-53 -- for the raw sequence's point 1
    (u - 0.5 = 2^-33 in every dimension) that rounding is 1e-6 of the value, ten float32 ulps, on EITHER side of a comparison.  So the
    yardstick is ndtri(0.5 + q) where float64 holds 0.5 + q to 2^-44 relative of q (|q| >= 2^-8), and below that the series of the
    quantile at the mode, sqrt(2 pi) (q + pi/3 q^3 + 7 pi^2/30 q^5 + 127 pi^3/630 q^7), whose next term is below 1e-17 relative there."""
    import torch
    u = uniforms(bits)
    if truncate is None:
        return torch.special.ndtri(torch.from_numpy(np.ascontiguousarray(u))).numpy()
    t = float(np.float32(truncate))
    lo, hi = (float(v) for v in torch.special.ndtr(torch.tensor([-t, t], dtype=torch.float64)))
    q = (u - 0.5) * (hi - lo)
    big = torch.special.ndtri(torch.from_numpy(np.ascontiguousarray(0.5 + q))).numpy()
    q2 = q * q
    small = np.sqrt(2.0 * np.pi) * q * (1.0 + q2 * (np.pi / 3.0 + q2 * (7.0 * np.pi ** 2 / 30.0 + q2 * (127.0 * np.pi ** 3 / 630.0))))
    return np.clip(np.where(np.abs(q) >= 2.0 ** -8, big, small), -t, t)


def is_net_1d(x, M):
    """Every dimension's top log2(M) bits of the first M points are a permutation of 0 .. M-1.  x: [M, zdim] uint32."""
    m = M.bit_length() - 1
    top = (x >> np.uint32(32 - m)).astype(np.int64) if m else np.zeros_like(x, dtype=np.int64)
    return all(np.array_equal(np.sort(top[:, d]), np.arange(M)) for d in range(x.shape[1]))


def is_net_2d(x0, x1, M):
    """(0, m, 2)-net: every elementary interval 2^-a x 2^-(m-a) holds exactly one of the M points."""
    m = M.bit_length() - 1
    for a in range(m + 1):
        i0 = (x0.astype(np.uint64) >> np.uint64(32 - a)) if a else np.zeros(M, np.uint64)
        i1 = (x1.astype(np.uint64) >> np.uint64(32 - (m - a))) if m - a else np.zeros(M, np.uint64)
        cell = i0 * np.uint64(1 << (m - a)) + i1
        if not np.array_equal(np.sort(cell.astype(np.int64)), np.arange(M)):
            return False
    return True
