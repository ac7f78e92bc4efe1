"""GPU: one segment table for every context (csrc/pp_segments.h).

A padded [B][L] context and a packed context whose table is 0, L, 2L ... over the same rows (``pack(split(padded), trim=False)``)
describe the same complexes: same ``seg``, K and N, so every per-complex quantity -- graph, score, seeded noise, noised angles, the
loss, a seeded sample -- must have the same BITS on both, and for one complex the padded B = 1 context, the packed one-segment
context, ``proximal`` and ``proximal_packed`` must agree bit for bit.  No tolerance anywhere: the two descriptions run the same
arithmetic or they do not."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SEED = 0x5e67_7ab1e
VTF, TOL, LAMDA = 12.0, 0.5, 1.0


@pytest.fixture(scope="module")
def plan(weights):
    from packppi_amd.lib import Plan
    return Plan(weights, torch.device(DEV))


def _pair(plan, lens):
    """(padded context, the context of the same rows packed under the uniform table, N)"""
    from packppi_amd import synth
    from packppi_amd.batch import collate, pack, split
    from packppi_amd.featurize import protein_to_data
    from packppi_amd.lib import Context
    padded = collate([protein_to_data(synth.make_complex(n, 90 + n)) for n in lens]).to(DEV)
    uniform = pack(split(padded), trim=False)
    B, L = len(lens), max(lens)
    assert uniform["seg_offsets_host"] == [s * L for s in range(B + 1)]
    a, b = Context(plan, padded), Context(plan, uniform)
    assert (a.B, a.L, b.B, b.L) == (B, L, 1, B * L) and a.K == b.K == min(32, L)
    assert a.n_segments == b.n_segments == B
    return padded, a, b, B * L


def _same(x, y):
    return x.shape.numel() == y.shape.numel() and torch.equal(x.reshape(-1), y.reshape(-1))


@pytest.mark.parametrize("lens", [(40, 52, 33), (17, 17)], ids=["B3_L52", "B2_L17_K17"])
def test_padded_and_uniform_table_contexts_have_the_same_bits(plan, lens):
    padded, a, b, N = _pair(plan, lens)
    g = torch.Generator().manual_seed(len(lens))
    chi = padded.SC_D
    for x, y in zip(a.graph(), b.graph()):                      # E_idx (per-complex numbering), h_E0
        assert _same(x, y)
    for x, y in zip(a.score(chi, 0.5), b.score(chi, 0.5)):
        assert _same(x, y)
    for keys in (None, [7, 5, 11][:len(lens)]):
        a.set_rng_keys(keys)
        b.set_rng_keys(keys)
        for step in (-1, 3):
            (nx, wx), (ny, wy) = a.noise(SEED, step, want_words=True), b.noise(SEED, step, want_words=True)
            assert torch.equal(nx, ny) and torch.equal(wx, wy), (keys, step)
        # two complexes with different keys draw different noise: the table, not the row number alone, keys a row
        assert keys is None or not torch.equal(nx[:, :a.L], nx[:, a.L:2 * a.L])
        xa, xb = a.add_noise(chi, 0.7, SEED), b.add_noise(chi, 0.7, SEED)
        assert _same(xa, xb)
    pred, target = torch.randn(N, 4, generator=g).to(DEV), torch.randn(N, 4, generator=g).to(DEV)
    t_rows = torch.rand(len(lens), generator=g).repeat_interleave(a.L).to(DEV)
    norm = (torch.rand(2, 5001, generator=g, dtype=torch.float64) + 0.25).to(DEV)
    for x, y in zip(a.dsm_loss(pred, target, t_rows, norm), b.dsm_loss(pred, target, t_rows, norm)):
        assert x.shape == (len(lens),) and torch.equal(x, y)
    sched = torch.linspace(1, 0, 4)
    sa, sb = a.sample(xa, sched, "sde", seed=SEED), b.sample(xb, sched, "sde", seed=SEED)
    assert _same(sa, sb) and not _same(sa, xa)


def test_one_complex_padded_packed_proximal_and_proximal_packed(plan):
    from packppi_amd import synth
    from packppi_amd.batch import pack
    from packppi_amd.featurize import protein_to_batch
    from packppi_amd.lib import Context
    batch = protein_to_batch(synth.make_complex(33, 123)).to(DEV)
    a, b = Context(plan, batch), Context(plan, pack([batch], trim=False))
    assert (a.B, a.L, b.B, b.L) == (1, 33, 1, 33) and b.n_segments == a.n_segments == 1
    chi = a.add_noise(batch.SC_D, 0.5, SEED)
    assert torch.equal(chi, b.add_noise(batch.SC_D, 0.5, SEED))
    _, last_a, loss_a = a.proximal(chi, VTF, TOL, LAMDA, 3)
    _, last_b, loss_b = b.proximal(chi, VTF, TOL, LAMDA, 3)
    assert torch.equal(last_a, last_b) and torch.equal(loss_a, loss_b)
    _, plast_a, acc_a, ploss_a = a.proximal_packed(chi, VTF, TOL, LAMDA, 3)
    _, plast_b, acc_b, ploss_b = b.proximal_packed(chi, VTF, TOL, LAMDA, 3)
    assert torch.equal(plast_a, plast_b) and torch.equal(acc_a, acc_b) and torch.equal(ploss_a, ploss_b)
    assert torch.equal(plast_a, last_a) and torch.equal(ploss_a[0], loss_a)
    ls = [float(v) for v in loss_a.cpu()]
    assert torch.equal(acc_a, last_a if ls[-1] < ls[0] else chi)
