"""The network at every launch-regime boundary and at the small end.

Which kernel instance each of the seven launches of a network evaluation runs depends on the context's row count N and the device's
compute-unit count C alone (pp_edge_f16.hip pick_R / use_mix / mix_pairs, pp_node.hip nu_shape).  Every size here is derived from C
as the device reports it; ``test_launch_plan_names_the_regimes`` asks the launchers (libpackppi_hip.dbg.so, pp_debug_launch_plan)
whether those sizes still sit where their labels say, so that a moved threshold moves the sweep instead of emptying it.

The arbiter is the fp32 CPU oracle, never the fp64 one: about one non-self edge in 12 000 has a pair dihedral whose arccos argument
rounds past -1 in fp32 (NaN -> 0, the reference's behaviour and the device's) and is +-3.1414 in fp64 (h_E0 moves by 1.0, the score
by 1e-3).  ``arccos_edges`` lists them and every assertion message carries the list.
"""
import ctypes as C
import functools
import os

import pytest
import torch

from .conftest import WEIGHT_SEED, load_golden, wrapped_absdiff

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SCHED = torch.linspace(1, 0, 3)          # two reverse steps: the in-sampling node update, the write-back-free layer-1 edge update
BOUNDARY = ["2C", "2C+1", "2C+2", "2C+3", "3C-1", "3C", "3C+1", "3C+2", "4C", "4C+1", "8C", "8C+1", "16C", "16C+1"]
ONE_COMPLEX_UP_TO = "4C+1"               # larger sizes run as packed batches only (synthesis of one complex grows too slow)
CASES = [(s, lay) for s in BOUNDARY[:BOUNDARY.index(ONE_COMPLEX_UP_TO) + 1] for lay in ("single", "packed3")] + \
        [(s, "packed315") for s in BOUNDARY[BOUNDARY.index(ONE_COMPLEX_UP_TO) + 1:]]
# (R, mixed, cl, multi) the labels stand for; n_pairs follows from N
REGIME = {"2C": (1, 0, 4, 0), "2C+1": (1, 1, 4, 0), "2C+2": (1, 1, 4, 0), "2C+3": (1, 1, 4, 0), "3C-1": (1, 1, 4, 0),
          "3C": (1, 1, 4, 0), "3C+1": (2, 0, 4, 0), "3C+2": (2, 0, 4, 0), "4C": (2, 0, 4, 0), "4C+1": (2, 0, 2, 0),
          "8C": (2, 0, 2, 0), "8C+1": (2, 0, 1, 0), "16C": (2, 0, 1, 0), "16C+1": (2, 0, 1, 1)}


def n_rows(label):
    """'3C+1' -> 3 * (compute units of device 0) + 1"""
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    mult, _, rest = label.partition("C")
    return int(mult) * cu + int(rest or 0)


@pytest.fixture(scope="module")
def model(weights):
    from packppi_amd.module import TDiffusionModule
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    return TDiffusionModule(weights, device=DEV)


@functools.lru_cache(maxsize=None)
def _weights():
    from packppi_amd.weights import make_random_state_dict
    return make_random_state_dict(WEIGHT_SEED)


def mask_out(b, rows):
    """tools/debug/fuzz_parity.py mask_out: what featurize.py does to a residue with a missing backbone atom, on a B = 1 batch"""
    for r in rows:
        b.residue_mask[0, r] = 0.0
        for k in ("X", "atom_mask", "SC_D", "SC_D_mask", "BB_D", "BB_D_mask", "BB_D_sincos", "SC_D_sincos"):
            b[k][0, r] = 0
        for k in ("chi_1pi_periodic_mask", "chi_2pi_periodic_mask"):
            b[k][0, r] = False


def arccos_edges(b, E_idx=None):
    """[(row, slot, neighbour, fp32 values of the dihedrals that differ)] of the non-self edges of a B = 1 batch with a pair dihedral
    (edge_features[..., 466:]) that differs by more than 1e-2 between the fp32 and the fp64 oracle."""
    from oracle import ref_cpu as O
    if E_idx is None:
        E_idx = O.knn_graph(b.X[:, :, 1, :], b.residue_mask)
    f32 = O.edge_features(b.X, E_idx, b.residue_index, b.chain_indices)[..., 466:]
    f64 = O.edge_features(b.X.double(), E_idx, b.residue_index, b.chain_indices)[..., 466:]
    L = E_idx.shape[1]
    differs = (f32.double() - f64).abs() > 1e-2
    bad = differs.any(-1) & (E_idx != torch.arange(L).view(1, L, 1))
    bad &= (b.residue_mask[0][E_idx] > 0) & (b.residue_mask[..., None] > 0)
    return [(r, k, int(E_idx[0, r, k]), tuple(f32[0, r, k][differs[0, r, k]].tolist())) for _, r, k in bad.nonzero().tolist()]


def static_on_device_lists(model, b):
    """(E_idx, h_E0) as O.encode_static, with the neighbour lists ``ctx.graph()`` returns.  The oracle's own search gives the same
    neighbours -- asserted -- but may order two of them differently: torch.sqrt on some CPUs is an ulp off the correctly rounded root
    the device takes (test_hip_parity.py::test_knn_ties_follow_the_reference_cpu_path), and per-edge tensors compare slot by slot."""
    from oracle import ref_cpu as O
    sd = _weights()
    E, hE = (x.cpu() for x in model._context(b.to(DEV)).graph())
    valid = b.residue_mask.bool()
    own = O.knn_graph(b.X[:, :, 1, :], b.residue_mask)
    assert torch.equal(E.sort(-1)[0][valid], own.sort(-1)[0][valid]), "the device's neighbour lists and the oracle's hold different residues"
    with torch.no_grad():
        feats = O.edge_features(b.X, E, b.residue_index, b.chain_indices)
        h_E0 = O._ln(O._linear(feats, sd["encoder.edge_embedding.weight"], sd["encoder.edge_embedding.bias"]),
                     sd["encoder.norm_edges.weight"], sd["encoder.norm_edges.bias"])
    return E, h_E0, hE


class Part:
    """One distinct complex of a case with what the oracle says about it, computed once per process and shared by the tests."""

    def __init__(self, n, seed, n_chains=2, masked=()):
        from oracle import ref_cpu as O
        from packppi_amd import synth
        from packppi_amd.featurize import protein_to_batch
        self.n = n
        self.b = protein_to_batch(synth.make_complex(n, seed, n_chains))
        mask_out(self.b, masked)
        with torch.no_grad():
            self.static = O.encode_static(_weights(), self.b)
        self.arccos = arccos_edges(self.b, self.static[0])
        self._net, self._ode = {}, {}

    def init(self, v):
        g = torch.Generator().manual_seed(977 * self.n + v)
        return (torch.rand(1, self.n, 4, generator=g) * 2 - 1) * 3.0 * self.b.SC_D_mask

    def t(self, v):
        return 0.4 + 0.1 * v

    def network(self, v):
        from oracle import ref_cpu as O
        if v not in self._net:
            with torch.no_grad():
                self._net[v] = O.network(_weights(), self.b, self.init(v), torch.full((self.n,), self.t(v)), self.static)
        return self._net[v]

    def sampled(self, v):
        from oracle import ref_cpu as O
        if v not in self._ode:
            with torch.no_grad():
                self._ode[v] = O.sampling(_weights(), self.b, self.init(v), SCHED, static=self.static)
        return self._ode[v]

    def sampled_sde(self, v, noise):
        from oracle import ref_cpu as O
        with torch.no_grad():
            return O.sampling(_weights(), self.b, self.init(v), SCHED, mode="sde", sde_noise=noise, static=self.static)


def three_lengths(n):
    """three near-equal lengths that sum to n, none a multiple of 16: 16-row tiles straddle both segment boundaries"""
    q = n // 3
    fits = [(q + a, q + b, n - 2 * q - a - b) for a in range(-2, 3) for b in range(-2, 3)]
    lens = min((x for x in fits if all(m % 16 for m in x)), key=lambda x: max(x) - min(x))
    assert sum(lens) == n and min(lens) >= 33, lens
    return list(lens)


class Case:
    """A context-sized batch: segments = [(part, variant)], each variant with its own initial angles and its own time."""

    def __init__(self, parts, segments, packed, trim=True):
        from packppi_amd.batch import pack
        self.parts, self.segments = parts, segments
        self.batch = pack([p.b for p, _ in segments], trim=trim) if packed else segments[0][0].b
        self.offs = [0]
        for p, _ in segments:
            self.offs.append(self.offs[-1] + p.n)
        self.n = self.offs[-1]
        self.chi = torch.cat([p.init(v) for p, v in segments], 1)
        self.t = torch.cat([torch.full((p.n,), p.t(v)) for p, v in segments])

    def rows(self):
        return list(zip(self.segments, self.offs[:-1], self.offs[1:]))

    def note(self):
        """what every assertion message ends with: the arccos edges of the case, in the numbering of the batch"""
        e = sorted({(a + r, a + j) for (p, _), a, _ in self.rows() for r, _, j, _ in p.arccos})
        return f"N = {self.n}, segments {[p.n for p, _ in self.segments]}; fp32-arccos edges (row, neighbour): {e or 'none'}"


@functools.lru_cache(maxsize=None)
def boundary_case(label, layout):
    n = n_rows(label)
    if layout == "single":
        p = Part(n, 100 + n)
        return Case([p], [(p, 0)], packed=False)
    if layout == "packed3":
        parts = [Part(m, 200 + n + k) for k, m in enumerate(three_lengths(n))]
        return Case(parts, [(p, k) for k, p in enumerate(parts)], packed=True)
    # at most two distinct complexes of about 315 rows, repeated; a copy has one of two variants (initial angles, time)
    count = max(1, n // 315)
    short, longer = n // count, n % count
    parts = [Part(short, 300 + short)] + ([Part(short + 1, 300 + short + 1)] if longer else [])
    order = [parts[(k * longer) // count != ((k + 1) * longer) // count] for k in range(count)]      # the longer ones spread evenly
    seen, segments = {}, []
    for p in order:
        segments.append((p, seen.get(p, 0) % 2))
        seen[p] = seen.get(p, 0) + 1
    case = Case(parts, segments, packed=True)
    assert case.n == n, (case.n, n)
    return case


def check_network(model, case):
    """|hV - oracle| < 1e-4, |score - oracle| < 5e-5 on valid rows (test_hip_parity.py::test_network)"""
    gb = case.batch.to(DEV)
    score, hV = model.network(gb, case.chi.to(DEV), case.t)
    score, hV = score.cpu(), hV.cpu()
    worst = [0.0, 0.0]
    for (p, v), a, e in case.rows():
        valid = p.b.residue_mask[0].bool()
        if not valid.any():
            continue
        s_o, h_o = p.network(v)
        dh, ds = (hV[0, a:e] - h_o[0])[valid].abs(), (score[0, a:e] - s_o[0])[valid].abs()
        worst = [max(worst[0], float(dh.max())), max(worst[1], float(ds.max()))]
        assert dh.max() < 1e-4, (f"h_V: {float(dh.max()):.2e} at row {a + int(valid.nonzero()[int(dh.max(-1)[0].argmax())])}", case.note())
        assert ds.max() < 5e-5, (f"score: {float(ds.max()):.2e} at row {a + int(valid.nonzero()[int(ds.max(-1)[0].argmax())])}", case.note())
    return worst


def check_sampling(model, case, mode="ode"):
    """two reverse steps, wrapped < 1e-4 rad on SC_D_mask (tools/debug/fuzz_parity.py)"""
    ctx = model._context(case.batch.to(DEV))
    noise = None
    if mode == "sde":
        noise = torch.randn(len(SCHED) - 1, 2, case.n, 4, generator=torch.Generator().manual_seed(case.n))
    out = ctx.sample(case.chi.to(DEV), SCHED, mode, noise).cpu()
    worst = 0.0
    for (p, v), a, e in case.rows():
        m = p.b.SC_D_mask[0].bool()
        if not m.any():
            continue
        ref = p.sampled(v) if mode == "ode" else p.sampled_sde(v, [(noise[j, 0, a:e], noise[j, 1, a:e]) for j in range(len(SCHED) - 1)])
        d = wrapped_absdiff(out[0, a:e], ref[0]) * m
        worst = max(worst, float(d.max()))
        assert d.max() < 1e-4, (f"{mode} sampling: {float(d.max()):.2e} rad at row {a + int(d.max(-1)[0].argmax())}", case.note())
        assert torch.equal(out[0, a:e][~m], torch.zeros_like(out[0, a:e][~m]))
    return worst, out


# ---- 1. the boundaries ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label,layout", CASES)
def test_boundary_network_and_sampling(label, layout, model):
    """One evaluation at t = 0.4 (a packed batch: a time per complex, through the per-row embedding) and two reverse steps, as one
    complex and as a packed batch whose 16-row tiles straddle the segment boundaries, against the fp32 oracle."""
    case = boundary_case(label, layout)
    dh, ds = check_network(model, case)
    dchi, _ = check_sampling(model, case)
    assert model.saturated() == 0
    print(f"boundary {label:6s} {layout:9s} N {case.n:5d}: dhV {dh:.2e}  dscore {ds:.2e}  dchi {dchi:.2e}   [{case.note()}]")


@pytest.mark.parametrize("label,layout", [("2C+1", "single"), ("2C+1", "packed3"), ("3C+1", "single"), ("3C+1", "packed3")])
def test_boundary_sde(label, layout, model):
    """mode = "sde" with one explicit noise tensor handed to both sides, in the mixed launch and in the first two-row one"""
    case = boundary_case(label, layout)
    dchi, _ = check_sampling(model, case, "sde")
    print(f"boundary {label:6s} {layout:9s} N {case.n:5d}: sde dchi {dchi:.2e}")


# ---- 2. the regimes are the ones named (libpackppi_hip.dbg.so: test_hip_layers.py::test_diag_library_runs_the_layer_tests) ----------
def _diag():
    from packppi_amd import lib as L
    l = L.load()
    if not hasattr(l, "pp_debug_launch_plan"):
        pytest.skip("needs libpackppi_hip.dbg.so (run through test_hip_layers.py::test_diag_library_runs_the_layer_tests)")
    l.pp_debug_launch_plan.argtypes = [C.c_void_p, C.c_void_p]
    l.pp_debug_score_prefix.argtypes = [C.c_void_p, C.c_void_p, C.c_float, C.c_int, C.c_void_p]
    l.pp_debug_buffer.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]
    return l


@pytest.mark.parametrize("label", BOUNDARY)
def test_launch_plan_names_the_regimes(label, model):
    """2C: one-row workgroups, not mixed; 2C+1 .. 3C: the mixed launch with ceil(N / 3) pair workgroups; from 3C+1: two rows per
    workgroup; middle-layer node updates 4 -> 2 workgroups per tile at 4C+1 and 2 -> 1 at 8C+1; the more-tiles-than-CUs instance from
    16C+1 -- answered by the predicates the launchers call."""
    l = _diag()
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    assert cu % 4 == 0, "the tile boundaries 4C, 8C, 16C are whole tiles only for a CU count that is a multiple of 4"
    n = n_rows(label)
    case = boundary_case(label, "packed3" if (label, "packed3") in CASES else "packed315")
    ctx = model._context(case.batch.to(DEV))
    out = (C.c_int32 * 5)()
    assert l.pp_debug_launch_plan(ctx.handle, out) == 0, l.pp_last_error()
    R, mixed, n_pairs, cl, multi = list(out)
    assert ctx.n_rows == n and (R, mixed, cl, multi) == REGIME[label], (label, n, list(out))
    if mixed:
        assert n_pairs == (n + 2) // 3 and 0 <= n - 2 * n_pairs <= n_pairs and n_pairs + (n - 2 * n_pairs) <= 2 * cu, (n, n_pairs)
    else:
        assert n_pairs == 0


AFTER = {"hV0": 1, "hV_l0": 3, "hE_l0": 4, "hV_l1": 5, "hE_l1": 6, "hV_l2": 7}      # test_hip_layers.py: launches before the tensor is in place


@pytest.mark.parametrize("label", ["2C+1", "3C", "3C+1"])
def test_per_layer_states_at_boundaries(label, model):
    """The tensors between the launches (test_hip_layers.py: h_V within 5e-5, h_E within 1e-4) against the oracle's own layer loop;
    the first launch and row that disagree are reported."""
    from oracle import ref_cpu as O
    l = _diag()
    case = boundary_case(label, "single")
    p, b, n = case.parts[0], case.parts[0].b, case.n
    sd = _weights()
    E_idx, h_E, _ = static_on_device_lists(model, b)
    with torch.no_grad():
        h_V = O.encode_nodes(sd, b, case.chi, case.t)
        ref = {"hV0": h_V}
        R, tr = O.backbone_frames(b.X)
        mask_att = b.residue_mask[..., None] * O._gather_nodes(b.residue_mask[..., None], E_idx)[..., 0]
        for layer in range(3):
            h_V, h_E = O.ipmp_layer(sd, layer, h_V, h_E, E_idx, R, tr, b.residue_mask, mask_att, edge_update=layer < 2)
            ref[f"hV_l{layer}"] = h_V
            if layer < 2:
                ref[f"hE_l{layer}"] = h_E
    ctx = model._context(b.to(DEV))
    chi = case.chi.to(DEV).contiguous()
    valid = b.residue_mask.bool()
    worst = {}
    for key, launches in AFTER.items():
        assert l.pp_debug_score_prefix(ctx.handle, C.c_void_p(chi.data_ptr()), float(case.t[0]), launches, None) == 0, l.pp_last_error()
        got = torch.empty((1, n, 128) if key.startswith("hV") else (1, n, ctx.K, 128), device=DEV)
        assert l.pp_debug_buffer(ctx.handle, 5 if key.startswith("hV") else 0, C.c_void_p(got.data_ptr()), got.numel()) == 0, l.pp_last_error()
        d = (got.cpu() - ref[key])[valid].abs().reshape(int(valid.sum()), -1).max(-1)[0]
        bound = 5e-5 if key.startswith("hV") else 1e-4
        worst[key] = float(d.max())
        assert d.max() < bound, (f"first disagreement after launch {launches} ({key}): row {int(valid[0].nonzero()[int((d >= bound).nonzero()[0])])}, "
                                 f"{float(d.max()):.2e} at worst", case.note())
    print(f"layers {label:6s} N {n}: " + "  ".join(f"{k} {v:.1e}" for k, v in worst.items()))


# ---- 3. small ends and segment edges ---------------------------------------------------------------------------------------------
def check_small(model, case, geometry=True):
    """network + two reverse steps, and for one complex atom14 / clash of the sampled angles (fuzz_parity: 5e-5 A, 1e-4)"""
    from oracle import ref_cpu as O
    from packppi_amd.functional import compute_residue_clash, get_atom14_coords
    dh, ds = check_network(model, case)
    dchi, out = check_sampling(model, case)
    dx = dc = 0.0
    if geometry:
        b, gb = case.batch, case.batch.to(DEV)
        xyz = get_atom14_coords(gb.X, gb.residue_type, gb.BB_D, out.to(DEV)).cpu()
        dx = float(((xyz - O.atom14_coords(b.X, b.residue_type, b.BB_D, out)) * b.atom_mask[..., None]).abs().max())
        cl = compute_residue_clash(gb, out.to(DEV), 12.0, 0.5).cpu()
        with torch.no_grad():
            dc = float(((cl - O.residue_clash(b, out, 12.0, 0.5)) * b.residue_mask).abs().max())
        assert torch.isfinite(xyz).all() and torch.isfinite(cl).all()
        assert dx < 5e-5 and dc < 1e-4, (dx, dc, case.note())
    assert model.saturated() == 0
    return f"dhV {dh:.2e}  dscore {ds:.2e}  dchi {dchi:.2e}  dxyz {dx:.2e}  dclash {dc:.2e}"


@pytest.mark.parametrize("L,n_chains", [(1, 1), (2, 1), (3, 1), (2, 2), (15, 2), (16, 2), (17, 2), (31, 2), (32, 2), (33, 2)])
def test_small_ends_single_complex(L, n_chains, model):
    """K = L below 32 rows, down to one residue: one tile with 15 dead rows, neighbour lists of one entry, a chain of one residue"""
    p = Part(L, 400 + 10 * L + n_chains, n_chains)
    print(f"small L {L} chains {n_chains}: " + check_small(model, Case([p], [(p, 0)], packed=False)))


def test_small_ends_padded_batch_1_5_3(model, weights):
    """A padded batch of lengths (1, 5, 3): K = 5, the padding rows of the shorter complexes are launched and masked."""
    from oracle import ref_cpu as O
    from packppi_amd import synth
    from packppi_amd.batch import collate
    from packppi_amd.featurize import protein_to_data
    b = collate([protein_to_data(synth.make_complex(n, 500 + n, 1)) for n in (1, 5, 3)])
    B, L = b.residue_type.shape
    assert (B, L) == (3, 5) and b.residue_mask.sum(1).tolist() == [1, 5, 3]
    init = (torch.rand(B, L, 4, generator=torch.Generator().manual_seed(153)) * 2 - 1) * 3.0 * b.SC_D_mask
    valid = b.residue_mask.bool()
    with torch.no_grad():
        s_o, h_o = O.network(weights, b, init, torch.full((B * L,), 0.4))
        ref = O.sampling(weights, b, init, SCHED)
    gb = b.to(DEV)
    score, hV = model.network(gb, init.to(DEV), torch.full((B * L,), 0.4))
    dh, ds = (hV.cpu() - h_o)[valid].abs().max(), (score.cpu() - s_o)[valid].abs().max()
    out = model._context(gb).sample(init.to(DEV), SCHED).cpu()
    dchi = wrapped_absdiff(out, ref)[b.SC_D_mask.bool()].max()
    print(f"padded (1, 5, 3): dhV {float(dh):.2e}  dscore {float(ds):.2e}  dchi {float(dchi):.2e}")
    assert dh < 1e-4 and ds < 5e-5 and dchi < 1e-4 and model.saturated() == 0


@pytest.mark.parametrize("rows", [(0,), (39,), (15, 16)])
def test_masked_rows_at_the_ends_of_a_complex(rows, model):
    """A 40-residue complex whose first row, last row, or rows 15 and 16 (the last of the first tile and the first of the second) are
    masked the way featurize.py masks a residue without backbone."""
    p = Part(40, 640, masked=rows)
    print(f"masked {rows}: " + check_small(model, Case([p], [(p, 0)], packed=False)))


def test_masked_rows_at_a_segment_boundary(model):
    """A packed batch with the last row of segment 0 and the first row of segment 1 masked (packed untrimmed: the masked last row
    stays a row of its segment)."""
    parts = [Part(40, 641, masked=(39,)), Part(50, 642, masked=(0,))]
    case = Case(parts, [(parts[0], 0), (parts[1], 1)], packed=True, trim=False)
    assert case.batch.seg_offsets_host == [0, 40, 90]
    print("masked at a segment boundary: " + check_small(model, case, geometry=False))


# ---- 4. the arccos edge itself -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["g3_sampling_L300", "complex_769_869"])
def test_arccos_edges_follow_the_fp32_oracle(which, model):
    """h_E0 of ``ctx.graph()`` on the edges whose pair dihedral is 0.0 in fp32 (arccos argument past -1: NaN -> 0) and +-3.14 in
    fp64, at test_graph's 2e-5 against the fp32 oracle -- after checking that the oracle on this machine still gives exactly 0.0
    there (an edge where it does not is left out, and named)."""
    from packppi_amd import synth
    from packppi_amd.featurize import protein_to_batch
    b = load_golden(which)[0] if which.startswith("g3") else protein_to_batch(synth.make_complex(769, 869))
    E_idx, h_E0, hE = static_on_device_lists(model, b)
    edges = arccos_edges(b, E_idx)
    valid = b.residue_mask.bool()
    real = (b.residue_mask[0][E_idx] > 0) & valid[..., None]
    d = (hE - h_E0).abs().max(-1)[0]
    assert len(edges) >= 1, "this structure no longer has an edge whose fp32 and fp64 dihedrals differ"
    kept = [(r, k, j) for r, k, j, vals in edges if all(v == 0.0 for v in vals)]
    for r, k, j, vals in edges:
        if (r, k, j) not in kept:
            print(f"{which}: the fp32 oracle on this machine gives {vals}, not 0.0, on edge ({r}, {j}): left out")
            real[0, r, k] = False
    print(f"{which}: {len(edges)} fp32-arccos edges {[(r, j) for r, _, j, _ in edges]}, dhE0 there "
          f"{[f'{float(d[0, r, k]):.2e}' for r, k, _ in kept]}; all real edges: dhE0 {float(d[real].max()):.2e}")
    for r, k, j in kept:
        assert d[0, r, k] < 2e-5, (r, k, j, float(d[0, r, k]))
    assert d[real].max() < 2e-5, edges
