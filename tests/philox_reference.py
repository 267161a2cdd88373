"""A numpy restatement of the device generator of the stochastic master step (csrc/philox.h, written from the algorithm's description,
not from that header). Not a test module: tests/test_stochastic_host.py pins it to Random123's known answers, the GPU tests compare
the kernels with it.

``philox4x32_10``   Philox4x32-10 (Salmon et al., SC'11), vectorised over leading dimensions.
``group_words``     the words of the groups of four of one sample's stream at one step:
                        counter = (g low, g high, step, subsequence),  key = (seed low, seed high ^ DOMAIN)
``uniforms``        u = ((w >> 8) + 0.5)·2^-24, the SUM ROUNDED TO fp32 as the kernel rounds it (it is exact below w >> 8 = 2^23 and
                    rounds to even above; u lies in [2^-25, 1]).
``normals``         the fp64 normals of those u: z0 = r cos θ, z1 = r sin θ with r = sqrt(−2 ln u0), θ = 2π u1; z2, z3 from words 2, 3.
``stochastic_rule`` the step's rule in the dtype of its arguments."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
DOMAIN = 0x53544F43
MASK32 = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """counter [..., 4], key [..., 2] (uint32, broadcast against each other) -> words [..., 4] uint32."""
    c = np.asarray(counter, dtype=np.uint64) & MASK32
    k = np.asarray(key, dtype=np.uint64) & MASK32
    c0, c1, c2, c3 = (c[..., i] for i in range(4))
    k0, k1 = k[..., 0], k[..., 1]
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2            # < 2^64: no wrap
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & MASK32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & MASK32
        k0, k1 = (k0 + np.uint64(W0)) & MASK32, (k1 + np.uint64(W1)) & MASK32
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), axis=-1).astype(np.uint32)


def group_words(seed: int, subsequence: int, step: int, n_groups: int, first_group: int = 0):
    """[n_groups, 4] uint32: the words of groups first_group .. first_group + n_groups − 1."""
    g = np.arange(first_group, first_group + n_groups, dtype=np.uint64)
    seed, subsequence = int(seed) & 0xFFFFFFFFFFFFFFFF, int(subsequence) & MASK32
    counter = np.stack([g & MASK32, g >> np.uint64(32), np.full_like(g, int(step) & MASK32), np.full_like(g, subsequence)], axis=-1)
    key = np.array([seed & MASK32, ((seed >> 32) & MASK32) ^ DOMAIN], dtype=np.uint64)
    return philox4x32_10(counter, key)


def uniforms(words):
    """float32, as the kernel forms it: (float)(w >> 8) is exact, + 0.5 rounds to fp32 once, · 2^-24 is exact."""
    k = (np.asarray(words, dtype=np.uint32) >> np.uint32(8)).astype(np.float32)
    return (k + np.float32(0.5)) * np.float32(2.0 ** -24)


def normals(words):
    """[..., 4] words -> [..., 4] float64 standard normals."""
    u = uniforms(words).astype(np.float64)
    out = np.empty(u.shape, dtype=np.float64)
    for a in (0, 2):
        r = np.sqrt(-2.0 * np.log(u[..., a]))
        theta = 2.0 * np.pi * u[..., a + 1]
        out[..., a], out[..., a + 1] = r * np.cos(theta), r * np.sin(theta)
    return out


def sample_normals(seed: int, subsequence: int, step: int, n_s: int):
    """[n_s] float64: z of every element of one sample at one step."""
    return normals(group_words(seed, subsequence, step, (n_s + 3) // 4)).reshape(-1)[:n_s]


def stochastic_rule(x, v, z, sigma: float, sigma_next: float, eta: float):
    """x0 = x − σ·v;  ê = x0 + v;  n = η < 1 ? sqrt(1 − η²)·ê + η·z : z;  r = (1 − σ')·x0 + σ'·n; σ' = 0: r = x0, z unused."""
    x0 = x - sigma * v
    if sigma_next == 0.0:
        return x0
    n = z if eta >= 1.0 else float(np.sqrt(1.0 - float(eta) ** 2)) * (x0 + v) + eta * z
    return (1.0 - sigma_next) * x0 + sigma_next * n
