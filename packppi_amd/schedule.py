"""The training-side pieces of the reference's ``SO2Schedule`` (src/models/components/schedule.py:30-94) without its tables.

``so2_score``         SO2Schedule.score(x, sigma): the entry of the 5001 x 5001 table is computed on the device (lib.so2_score).
``score_norm_tables`` SO2Schedule.score_norm_ of the 1pi and the 2pi schedule.

``score_norm_`` is a Monte-Carlo estimate from UNSEEDED ``np.random`` (schedule.py:23-26, 57-63): 10000 draws per grid sigma,
so every entry carries about 1.4 % of sampling noise and the reference's loss differs between processes by about a percent.
``score_norm_tables(seed)`` makes the reference's draws in the reference's order, so a seed gives the table it gives the
reference (up to the few samples per column whose fp32 log lands on the other side of a rounding boundary); every consumer
also takes a table from the caller (``np.save`` of ``np.stack([m.schedule_1pi_periodic.score_norm_,
m.schedule_2pi_periodic.score_norm_])`` from a reference run).
"""
import numpy as np
import torch

from .lib import SO2_GRID, so2_grids, so2_score  # noqa: F401

N_DRAWS = 10000


def score_norm_tables(seed=None, device="cuda", rows_per_launch=500) -> np.ndarray:
    """-> float64 [2, 5001] (1pi schedule, then 2pi).  ``seed``: ``np.random.seed(seed)`` first; None keeps the global stream
    as it is (the reference's behaviour).  Needs about 1 GB of host memory for the 10000 x 5001 draws of one schedule."""
    if seed is not None:
        np.random.seed(seed)
    device = torch.device(device)
    _, sigma_grids = so2_grids()
    out = []
    for pi_periodic, PI, sigma in ((True, 1 / 2 * np.pi, sigma_grids[0]), (False, np.pi, sigma_grids[1])):
        sig = sigma[None].repeat(N_DRAWS, 0).flatten()                       # schedule.py:58-60
        x = sig * np.random.randn(*sig.shape)                                # sample(): one draw of 10000 * 5001
        x = ((x + PI) % (2 * PI) - PI).reshape(N_DRAWS, SO2_GRID)
        sig_dev = torch.from_numpy(sigma).to(device)
        acc = torch.zeros(SO2_GRID, dtype=torch.float64, device=device)
        for r in range(0, N_DRAWS, rows_per_launch):
            xs = torch.from_numpy(x[r:r + rows_per_launch]).to(device)
            s = so2_score(xs, sig_dev[None], pi_periodic)
            acc += (s.double() ** 2).sum(0)
        out.append((acc / N_DRAWS).cpu().numpy())
    return np.stack(out)


def load_score_norm(tables) -> np.ndarray:
    """A caller's table: an ``.npy`` path or an array-like [2, 5001] -> float64 array, validated."""
    if isinstance(tables, torch.Tensor):
        tables = tables.detach().cpu().numpy()
    arr = np.load(tables) if isinstance(tables, (str, bytes)) or hasattr(tables, "__fspath__") else tables
    arr = np.asarray(arr, dtype=np.float64)
    if arr.shape != (2, SO2_GRID) or not np.isfinite(arr).all() or (arr < 0).any():
        raise ValueError(f"score_norm tables must be [2, {SO2_GRID}] finite non-negative numbers (1pi schedule, then 2pi), got {arr.shape}")
    return arr
