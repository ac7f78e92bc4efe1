"""Seeded, packing-invariant sampling noise generated on the device (csrc/pp_rng.h).

The generator is restated here in NumPy (Philox4x32-10, the counter layout, the uniform and the Box-Muller transform); the
device's raw words are held to it bit for bit, its normals to the fp64 evaluation of the same formula, the in-kernel draws of
pp_sample_seeded to the explicit-noise path on the exported draws, and the sampler to what the feature is for: a complex gets
the same angles alone, anywhere in a packed batch and on any shard layout.

Complexes: L = 33 (the smallest K = 32 complex, one row beyond two 16-row tiles), 40 and 64; packed N = 137 is no multiple of
the tile, so tiles hold rows of two complexes.  The large pack (14 x 300 rows + the three) has more 16-row tiles than the chip
has CUs, which is when the node update launches its shallow-ring instance."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from .conftest import wrapped_absdiff

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x1234_5678_9abc_def0
LENS = (33, 40, 64)
KEYS = (7, 2 ** 40 + 3, 11)
SCHED = torch.linspace(1, 0, 4)
gpu = pytest.mark.gpu

# ---- the generator, restated -------------------------------------------------------------------------------------------------
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)


def philox(counter, key):
    """Philox4x32-10 on arrays: counter = 4 words, key = 2 words -> 4 uint64 arrays holding 32-bit words."""
    c = [np.asarray(x, dtype=np.uint64) for x in counter]
    k = [np.uint64(key[0]), np.uint64(key[1])]
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [((p1 >> np.uint64(32)) ^ c[1] ^ k[0]) & _MASK, p1 & _MASK, ((p0 >> np.uint64(32)) ^ c[3] ^ k[1]) & _MASK, p0 & _MASK]
        k = [(k[0] + np.uint64(W0)) & _MASK, (k[1] + np.uint64(W1)) & _MASK]
    return c


def words(seed, lens, keys, step):
    """uint32 [N, 4, 4]: the four words of every (row, chi) of complexes of these lengths and keys packed back to back."""
    row = np.concatenate([np.arange(n, dtype=np.uint64) for n in lens])
    ckey = np.concatenate([np.full(n, k, dtype=np.uint64) for n, k in zip(lens, keys)])
    row, ckey = np.repeat(row, 4), np.repeat(ckey, 4)
    g = np.tile(np.arange(4, dtype=np.uint64), len(row) // 4)
    c1 = (np.uint64(4 * (step + 1)) + g) & _MASK
    o = philox([row, c1, ckey & _MASK, ckey >> np.uint64(32)], [seed & 0xFFFFFFFF, seed >> 32])
    return np.stack(o, -1).astype(np.uint32).reshape(-1, 4, 4)


def normals64(w):
    """fp64 [2, N, 4] from words [N, 4, 4]: u = ((o >> 9) + 0.5) 2^-23 (exact), z = sqrt(-2 ln u1) cos(2 pi u2)."""
    u = ((w >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23
    z = lambda a, b: np.sqrt(-2.0 * np.log(u[..., a])) * np.cos(2.0 * np.pi * u[..., b])
    return np.stack([z(0, 1), z(2, 3)])


def test_philox_known_answers():
    h = lambda v: " ".join("%08x" % int(x) for x in v)
    assert h(philox([0, 0, 0, 0], [0, 0])) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    assert h(philox([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2)) == "408f276d 41c83b0e a20bc7c6 6d5451fd"
    assert h(philox([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], [0xA4093822, 0x299F31D0])) == "d16cfe09 94fdcceb 5001e420 24126ea1"
    w = words(SEED, LENS, KEYS, -1)
    assert w.shape == (137, 4, 4) and np.array_equal(w[33:73], words(SEED, (40,), (KEYS[1],), -1))      # rows count within the complex


def test_moments_of_the_restated_normals():
    """33 976 values (steps -1 .. 29, N = 137, both schedules): 5-sigma bounds on mean, variance and the 1pi / 2pi correlation."""
    z = np.stack([normals64(words(SEED, LENS, KEYS, s)) for s in range(-1, 30)])
    n = z.size
    assert n == 33976 and np.abs(z).max() <= 5.8
    assert abs(z.mean()) < 5 / np.sqrt(n)
    assert abs(z.var() - 1) < 5 * np.sqrt(2 / n)
    assert abs(np.corrcoef(z[:, 0].ravel(), z[:, 1].ravel())[0, 1]) < 5 / np.sqrt(n / 2)


# ---- device ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(weights):
    from packppi_amd.module import TDiffusionModule
    m = TDiffusionModule(weights, device=DEV)
    m.schedule = SCHED
    return m


@pytest.fixture(scope="module")
def complexes():
    """The three complexes on the device, each carrying its key."""
    from packppi_amd import synth
    from packppi_amd.featurize import protein_to_batch
    cs = [protein_to_batch(synth.make_complex(n, 70 + n)).to(DEV) for n in LENS]
    for c, k in zip(cs, KEYS):
        c["complex_key"] = k
        c["complex_keys"] = [k]
    return cs


@pytest.fixture(scope="module")
def large(complexes):
    """(packed batch, keys): 14 complexes of 300 residues and the three small ones, 4337 rows."""
    from packppi_amd import synth
    from packppi_amd.batch import pack
    from packppi_amd.featurize import protein_to_batch
    two = [protein_to_batch(synth.make_complex(300, 900 + i)).to(DEV) for i in range(2)]
    pb = pack([two[i % 2] for i in range(14)] + list(complexes))
    keys = [100 + i for i in range(14)] + list(KEYS)
    assert pb.max_size == 14 * 300 + 137 > 16 * torch.cuda.get_device_properties(0).multi_processor_count
    return pb, keys


def _ctx(model, batch, keys):
    from packppi_amd.lib import Context
    ctx = Context(model._plan, batch)
    ctx.set_rng_keys(keys)
    return ctx


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


@gpu
def test_words_equal_the_restatement(model, complexes):
    from packppi_amd.batch import pack
    packed = _ctx(model, pack(complexes), KEYS)
    solo = [_ctx(model, c, [k]) for c, k in zip(complexes, KEYS)]
    for step in (-1, 0, 2):
        assert np.array_equal(_u32(packed.noise(SEED, step, want_words=True)[1]), words(SEED, LENS, KEYS, step))
        for ctx, n, k in zip(solo, LENS, KEYS):
            assert np.array_equal(_u32(ctx.noise(SEED, step, want_words=True)[1]), words(SEED, (n,), (k,), step))
    # without keys a complex's key is its ordinal; set_rng_keys(None) goes back to that
    packed.set_rng_keys(None)
    assert np.array_equal(_u32(packed.noise(SEED, 0, want_words=True)[1]), words(SEED, LENS, (0, 1, 2), 0))


@gpu
def test_normals_against_fp64(model, complexes):
    """|device - fp64| <= 1e-5: |z| <= 5.8 and the rounding of 6.2831855f u2 (<= 2.4e-7 in the argument) give 1.4e-6, the
    distance of 6.2831855f from 2 pi (1.7e-7 relative) as much again, logf / cosf / sqrtf a few ulp of a value below 5.8."""
    from packppi_amd.batch import pack
    ctx = _ctx(model, pack(complexes), KEYS)
    base = None
    for step in (-1, 0, 2):
        nz, w = ctx.noise(SEED, step, want_words=True)
        err = np.abs(nz.cpu().numpy().astype(np.float64) - normals64(_u32(w))).max()
        print(f"step {step}: max |device - fp64| = {err:.3g}")
        assert nz.shape == (2, 137, 4) and err <= 1e-5
        base = nz if step == 0 else base
    # another seed, another key, another step: every value changes
    assert (ctx.noise(SEED + 1, 0) != base).all() and (ctx.noise(SEED, 1) != base).all()
    ctx.set_rng_keys([k + 1 for k in KEYS])
    assert (ctx.noise(SEED, 0) != base).all()


def _seeded_vs_explicit(ctx):
    init = ctx.add_noise(ctx._t["SC_D"], 1.0, SEED)
    n_steps = len(SCHED) - 1
    seeded = ctx.sample(init, SCHED, "sde", seed=SEED)
    stack = torch.stack([ctx.noise(SEED, j) for j in range(n_steps)])
    assert stack.shape == (n_steps, 2, ctx.n_rows, 4)
    explicit = ctx.sample(init, SCHED, "sde", sde_noise=stack)
    assert torch.isfinite(seeded).all() and torch.equal(seeded, explicit)
    ode = ctx.sample(init, SCHED, "ode")
    assert torch.equal(ctx.sample(init, SCHED, "ode", seed=SEED), ode)
    assert not torch.equal(ode, seeded)                     # the noise did enter


@gpu
@pytest.mark.parametrize("case", ["L33", "pack137", "large"])
def test_in_kernel_draws_are_the_explicit_noise_path(case, model, complexes, large):
    """pp_sample_seeded (sde) == pp_sample on the stack of pp_noise_seeded(step = 0 .. n - 1), bit for bit; ode: == pp_sample."""
    from packppi_amd.batch import pack
    if case == "L33":
        ctx = _ctx(model, complexes[0], [KEYS[0]])
    elif case == "pack137":
        ctx = _ctx(model, pack(complexes), KEYS)
    else:
        ctx = _ctx(model, *large)
    _seeded_vs_explicit(ctx)


@gpu
def test_initial_noising(model, complexes):
    """add_noise == the torch formula of add_sc_noise on the step = -1 export, within 2e-6 wrapped; no noise outside the masks."""
    from packppi_amd.batch import pack
    pb = pack(complexes)
    ctx = _ctx(model, pb, KEYS)
    got = ctx.add_noise(pb.SC_D, 1.0, SEED)
    z = ctx.noise(SEED, -1)
    x = pb.SC_D.reshape(-1, 4)
    m1, m2 = pb.chi_1pi_periodic_mask.reshape(-1, 4), pb.chi_2pi_periodic_mask.reshape(-1, 4)
    sig = model._t_to_sigma(torch.ones(x.shape[0], device=x.device)).unsqueeze(-1)
    want = x + (z[0] * sig) * m1
    want = want + (z[1] * sig) * m2
    want = (want + np.pi) % (2 * np.pi) - np.pi
    d = wrapped_absdiff(got.reshape(-1, 4).cpu(), want.cpu())
    print(f"max wrapped |add_noise - torch formula| = {d.max().item():.3g}")
    assert d.max() <= 2e-6
    outside = ~(m1 | m2)
    assert outside.any() and torch.equal(got.reshape(-1, 4)[outside], x[outside])
    assert (got.reshape(-1, 4)[~outside] != x[~outside]).all()


def _set_mode(model, mode):
    model.hparams.sample_cfg.mode = mode


@gpu
@pytest.mark.parametrize("mode", ["ode", "sde"])
def test_packing_invariance(mode, model, complexes):
    """The feature: sampling(seed=5) gives every complex the same bits alone, in the pack [A, B, C] and in the pack [C, A, B];
    sample_sharded(seed=5) the same chis per complex id whatever world, rank and max_rows make of the groups."""
    from packppi_amd.batch import pack, unpack
    from packppi_amd.parallel import sample_sharded
    _set_mode(model, mode)
    try:
        alone = [model.sampling(c, seed=5) for c in complexes]
        pb = pack(complexes)
        assert pb["complex_keys"] == list(KEYS)
        abc = unpack(pb, model.sampling(pb, seed=5))
        order = (2, 0, 1)
        pc = pack([complexes[i] for i in order])
        assert pc["complex_keys"] == [KEYS[i] for i in order]
        cab = dict(zip(order, unpack(pc, model.sampling(pc, seed=5))))
        for i in range(3):
            assert torch.isfinite(alone[i]).all()
            assert torch.equal(alone[i], abc[i]) and torch.equal(alone[i], cab[i])
        assert not torch.equal(model.sampling(pb, seed=6), model.sampling(pb, seed=5))
        # sharded: the key of a complex is its global id
        plain = [type(c)({k: v for k, v in c.items() if not k.startswith("complex_key")}) for c in complexes]
        runs = {}
        for world, max_rows in ((1, 200_000), (2, 200_000), (3, 200_000), (1, 80), (1, 60)):
            chis = {}
            for rank in range(world):
                part, ids, rows = sample_sharded(model, plain, rank=rank, world=world, max_rows=max_rows, seed=5)
                assert torch.isfinite(rows).all()
                chis.update(part)
            runs[(world, max_rows)] = chis
        first = runs[(1, 200_000)]
        assert sorted(first) == [0, 1, 2]
        for chis in runs.values():
            assert all(torch.equal(chis[i], first[i]) for i in range(3))
        for i, c in enumerate(plain):                        # ... and it is what the complex gets alone under that key
            solo = type(c)(c)
            solo["complex_keys"] = [i]
            assert torch.equal(model.sampling(solo, seed=5), first[i])
    finally:
        _set_mode(model, "ode")


@gpu
def test_seeded_sde_sampling_allocates_no_noise_buffer(model, large):
    """100 seeded sde steps on the large pack: torch's peak rises by less than 8 chi-sized tensors (the explicit path's noise
    buffer alone is 200 of them)."""
    pb, keys = large
    pb = type(pb)(pb)
    pb["complex_keys"] = keys
    _set_mode(model, "sde")
    model.schedule = torch.linspace(1, 0, 101)
    try:
        model._context(pb)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = model.sampling(pb, seed=5)
        torch.cuda.synchronize()
        rise = torch.cuda.max_memory_allocated() - base
    finally:
        _set_mode(model, "ode")
        model.schedule = SCHED
    chi_bytes = pb.max_size * 4 * 4
    print(f"peak rise {rise} bytes = {rise / chi_bytes:.2f} chi-sized tensors")
    assert torch.isfinite(out).all() and rise < 8 * chi_bytes


@gpu
def test_exact_fp32_library():
    """The in-kernel path and the packing invariance once more on the exact-fp32 library (one child run under PACKPPI_LIB)."""
    from packppi_amd.build import other_variant_path
    lib = other_variant_path()
    if os.environ.get("PACKPPI_LIB"):
        pytest.skip("already a child run")
    if not os.path.exists(lib):
        pytest.skip(f"{os.path.basename(lib)} not built (__graft_entry__.build() builds it)")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider",
                        "-k", "test_in_kernel_draws_are_the_explicit_noise_path or test_packing_invariance"],
                       env=dict(os.environ, PACKPPI_LIB=lib), cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert "5 passed" in r.stdout


@gpu
def test_surface(model, complexes, tmp_path):
    from packppi_amd import synth
    from packppi_amd.cli import eval_diffusion
    from packppi_amd.parallel import sample_sharded
    from packppi_amd.pdb_io import to_pdb
    c = complexes[0]
    with pytest.raises(ValueError, match="exclude each other"):
        model.sampling(c, seed=1, sde_noise=torch.zeros(3, 2, 33, 4, device=DEV))
    with pytest.raises(ValueError, match="exclude each other"):
        sample_sharded(model, list(complexes), seed=1, init_chi={i: torch.zeros(1, n, 4) for i, n in enumerate(LENS)})
    with pytest.raises(ValueError, match="complex keys"):
        model._context(c).set_rng_keys([1, 2])
    pdb = tmp_path / "complex.pdb"
    pdb.write_text(to_pdb(synth.make_complex(60, 21)))
    out = {}
    for name, seed in (("a", 3), ("b", 3), ("c", 4)):
        eval_diffusion.main(["--input", str(pdb), "--outdir", str(tmp_path / name), "--molprobity_clash_loc", "/nonexistent",
                             "--device", "cuda", "--random_weights", "3", "--steps", "4", "--seed", str(seed)])
        out[name] = (tmp_path / name / "structure.pdb").read_bytes()
    assert out["a"] == out["b"] and out["a"] != out["c"]
