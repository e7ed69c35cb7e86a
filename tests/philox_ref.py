"""NumPy restatement of the indexed draws (include/dxmi_hip.h: dxmi_randn_indexed / dxmi_randint_indexed), shared by
test_random_util_host.py and test_hip_randn_indexed.py.  Philox-4x32-10 as published (Salmon et al., SC'11): integer arithmetic, so
the words are exact; the normals are formed in float64 from the same (exactly representable) uniforms."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """ctr: uint32 [..., 4], key: uint32 [..., 2] (broadcast against ctr) -> uint32 [..., 4]."""
    c = [np.asarray(ctr[..., i], dtype=np.uint64) for i in range(4)]
    k = [np.asarray(key[..., i], dtype=np.uint64) for i in range(2)]
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & MASK]
        k = [(k[0] + np.uint64(W0)) & MASK, (k[1] + np.uint64(W1)) & MASK]
    return np.stack(c, axis=-1).astype(np.uint32)


def words(indices, per_sample, seed, draw):
    """The raw 32-bit words of rows with the given global indices: uint32 [N, per_sample].  counter = (element / 4, draw, index low
    word, index high word), key = the two halves of the seed."""
    idx = np.asarray(indices, dtype=np.uint64).reshape(-1, 1)
    nblk = (per_sample + 3) // 4
    ctr = np.empty((len(idx), nblk, 4), dtype=np.uint32)
    ctr[..., 0] = np.arange(nblk, dtype=np.uint32)[None, :]
    ctr[..., 1] = np.uint32(draw)
    ctr[..., 2] = (idx & MASK).astype(np.uint32)
    ctr[..., 3] = (idx >> np.uint64(32)).astype(np.uint32)
    seed = int(seed) & ((1 << 64) - 1)
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint32)
    return philox4x32_10(ctr, key).reshape(len(idx), nblk * 4)[:, :per_sample]


def uniforms(w):
    """((x >> 9) + 0.5) 2^-23 in fp32 arithmetic, as the kernel forms it; exact, so float64 of it loses nothing."""
    u = ((w >> np.uint32(9)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -23)
    assert u.dtype == np.float32
    return u


def normals64(indices, per_sample, seed, draw):
    """float64 Box-Muller on the kernel's uniforms: pairs (x0, x1) and (x2, x3) of every block -> [N, per_sample]."""
    nblk = (per_sample + 3) // 4
    u = uniforms(words(indices, nblk * 4, seed, draw))
    assert np.array_equal(u.astype(np.float64).astype(np.float32), u) and u.min() > 0 and u.max() < 1
    u = u.astype(np.float64).reshape(len(u), nblk * 2, 2)
    r, th = np.sqrt(-2.0 * np.log(u[..., 0])), 2.0 * np.pi * u[..., 1]
    z = np.stack([r * np.cos(th), r * np.sin(th)], axis=-1)
    return z.reshape(len(z), nblk * 4)[:, :per_sample]
