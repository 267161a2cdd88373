"""The stochastic step in the oracle's loop. Not a test module: tests/test_stochastic_gpu.py runs
``loop_reference.denoise_loop_reference`` with the oracle's ``euler_step`` replaced, for the duration of the call, by the rule of the
stochastic master step fed the restatement's noise (tests/philox_reference.py) — the loop itself is not edited.

    x0 = x − σ·v;   ê = x0 + v;   n = η < 1 ? sqrt(1 − η²)·ê + η·z : z;   r = (1 − σ')·x0 + σ'·n          (σ' = 0: r = x0)

z of sample b at a step: the stream (seed_b, subsequence_b) at the step's ABSOLUTE index, which is the position of σ in the full sigma
table (a repaint that starts at t_start walks ``sigmas[t_start:]`` and draws what the full run draws there)."""
import contextlib

import torch

import philox_reference as ph
from oracle import flux_oracle as orc


@contextlib.contextmanager
def stochastic_euler_step(sigmas, rng_rows, eta: float):
    """``rng_rows``: (seed, subsequence) per sample of the latents' batch. The state is fp32, like the oracle's Euler step."""
    table = [float(s) for s in sigmas]
    assert len(set(table)) == len(table)

    def step(x, v, sigma, sigma_next):
        i = table.index(float(sigma))
        assert table[i + 1] == float(sigma_next) and x.shape[0] == len(rng_rows)
        n_s = x[0].numel()
        z = torch.stack([torch.from_numpy(ph.sample_normals(seed, sub, i, n_s)).to(torch.float32).reshape(x.shape[1:]) for seed, sub in rng_rows])
        return ph.stochastic_rule(x.float(), v.float(), z, float(sigma), float(sigma_next), float(eta)).to(v.dtype)

    real, orc.euler_step = orc.euler_step, step
    try:
        yield
    finally:
        orc.euler_step = real
