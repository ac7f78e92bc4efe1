"""GPU: the lazy workspaces of a context (pp_ctx_workspace in csrc/pp_internal.h).

pp_disulfide_close, pp_polar, pp_clashscore and pp_hnet_optimize each keep one allocation per context, made by their first call
and found again by every later one.  All four run on ONE context of 64 rows, then on a context of 24 rows (a fresh allocation of
another size while the first context's are alive), then on the first context again.  The second pass over a context must give the
bytes of the first, and the 24-row context the bytes of another fresh context of the same batch.  That shows the calls still work
in this order; it cannot show WHICH path a call took (a reallocation gives the same bytes), nor catch every mix-up of workspaces.
Which allocation is reused, replaced or freed is what tests/native/workspace_sanitize.cpp checks, on the host."""
import numpy as np
import pytest
import torch

from . import polar_oracle as O
from .test_allatom_gpu import new_ctx
from .test_hnet_gpu import seeded_chi

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

ENTRIES = (("pp_disulfide_close", lambda c, x: c.disulfides(chi=x)), ("pp_polar", lambda c, x: c.polar(chi=x)),
           ("pp_clashscore", lambda c, x: c.clashscore(chi=x)), ("pp_hnet_optimize", lambda c, x: c.hbond_optimize(chi=x)))


def run_all(ctx, chi):
    """{entry: {output: bytes}} of the four entries on the context, in the order of the workspace table."""
    out = {}
    for name, call in ENTRIES:
        res = call(ctx, chi)
        out[name] = {k: v.cpu().numpy().tobytes() for k, v in res.items() if torch.is_tensor(v)}
        assert out[name], name
    return out


def test_every_entry_finds_its_own_workspace_again():
    big, small = O.batch("c64"), O.batch("c24")
    chi_big, chi_small = seeded_chi(big).to(DEV), seeded_chi(small).to(DEV)
    a = new_ctx(big)
    first = run_all(a, chi_big)
    fresh = run_all(new_ctx(small), chi_small)
    again = run_all(a, chi_big)
    other = run_all(new_ctx(small), chi_small)
    for name, _ in ENTRIES:
        assert first[name].keys() == again[name].keys() and fresh[name].keys() == other[name].keys()
        for k in first[name]:
            assert first[name][k] == again[name][k], (name, k, "second pass over the 64-row context")
            assert fresh[name][k] == other[name][k], (name, k, "two fresh 24-row contexts")
    assert a.saturated() == 0
    # not vacuous: the two sizes really differ and the hydrogen-bond optimiser had movers
    assert len(first["pp_polar"]["res"]) != len(fresh["pp_polar"]["res"])
    assert (np.frombuffer(first["pp_hnet_optimize"]["state"], np.int32) >= 0).any()
