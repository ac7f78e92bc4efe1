"""Sharding independent complexes over the GPUs of a node.

The sampling path has no cross-complex term (``network`` is per batch row; ``proximal_optimizer`` asserts B == 1),
so complexes are dealt to ranks, every rank runs the whole path on its own shard, and the ONLY collective is an
all-gather of fixed-width per-complex metric rows (RCCL over xGMI when the process group backend is "nccl";
KB-sized, latency bound).  One process per GPU, launched by ``torchrun``.
"""
from typing import Dict, List, Sequence, Tuple

import torch
import torch.distributed as dist

METRIC_KEYS = tuple(f"chi_{i}_{s}" for i in range(4) for s in ("ae_rad", "ae_deg", "acc")) + ("atom_rmsd",)


def shard_complexes(lengths: Sequence[int], world_size: int) -> List[List[int]]:
    """Longest-processing-time-first assignment of complex indices to ranks (cost ~ residues)."""
    order = sorted(range(len(lengths)), key=lambda i: (-int(lengths[i]), i))
    load = [0] * world_size
    out: List[List[int]] = [[] for _ in range(world_size)]
    for i in order:
        r = min(range(world_size), key=lambda k: (load[k], k))
        out[r].append(i)
        load[r] += int(lengths[i])
    return [sorted(s) for s in out]


def metrics_to_row(metric: Dict[str, torch.Tensor]) -> torch.Tensor:
    return torch.stack([torch.as_tensor(metric[k], dtype=torch.float32).reshape(()) for k in METRIC_KEYS])


def packed_metric_rows(model, pb, chi, sizes) -> torch.Tensor:
    """``analyze_samples`` (TorsionalDiffusion.py:311-341) for every complex of a packed batch at once: one atom14 launch
    and segment sums instead of one context, one launch and a dozen small reductions per complex.  ``sizes`` = the complexes'
    own ``max_size`` (the reference's atom_rmsd denominator adds eps for every atom slot of the complex, padding included).
    Returns [n_complexes, len(METRIC_KEYS)] on the batch's device, rows in packing order."""
    import numpy as np
    offs = pb["seg_offsets_host"]
    n = len(offs) - 1
    dev = chi.device
    lens = torch.tensor([b - a for a, b in zip(offs[:-1], offs[1:])], device=dev)
    seg = torch.repeat_interleave(torch.arange(n, device=dev), lens)              # complex of every packed row

    def seg_sum(x):                                                                  # [1, N, ...] -> [n] sums per complex
        x = x.reshape(x.shape[1], -1).sum(-1)
        return torch.zeros(n, device=dev, dtype=x.dtype).index_add_(0, seg, x)

    true, m, pi1 = pb["SC_D"], pb["SC_D_mask"], pb["chi_1pi_periodic_mask"]
    cols = []
    for i in range(4):
        cnt = seg_sum(m[..., i])
        cnt = torch.where(cnt != 0, cnt, torch.ones_like(cnt))
        diff = (chi[..., i] - true[..., i]).abs()
        acc = torch.logical_and(diff * 180 / np.pi < 20, diff > 0).float()
        ae = torch.minimum(diff, 2 * np.pi - diff)
        ae = torch.where(pi1[..., i], torch.minimum(ae, np.pi - ae), ae)
        cols += [seg_sum(ae) / cnt, seg_sum(ae * 180 / np.pi) / cnt, seg_sum(acc) / cnt]
    pred = model.get_atom14_coords(pb, chi)
    w = pb["atom_mask"] * pb["residue_mask"][..., None]
    num = seg_sum(torch.sum((pb["X"] - pred) ** 2, dim=-1) * w)
    den = seg_sum(w) + model.eps * 14.0 * torch.tensor([float(sz) for sz in sizes], device=dev)
    cols.append(num / den)
    return torch.stack(cols, 1)


def gather_metric_rows(ids: torch.Tensor, rows: torch.Tensor, group=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """All-gather ragged (ids [n_r], rows [n_r, W]) from every rank; returns them sorted by complex id.

    Counts are exchanged first so each rank pads its block to the maximum; works for gloo (CPU tensors) and
    nccl/RCCL (device tensors) alike."""
    if not dist.is_available() or not dist.is_initialized():
        order = torch.argsort(ids)
        return ids[order], rows[order]
    world = dist.get_world_size(group)
    dev = rows.device
    n = torch.tensor([ids.numel()], device=dev, dtype=torch.int64)
    counts = [torch.zeros_like(n) for _ in range(world)]
    dist.all_gather(counts, n, group=group)
    counts = [int(c) for c in torch.cat(counts).tolist()]            # one read-back for all ranks
    cap = max(max(counts), 1)
    W = rows.shape[1] if rows.dim() == 2 else len(METRIC_KEYS)
    # ids travel as int64 in their own block (a float32 column is exact to 2^24 only), the rows as float32
    id_block = torch.zeros(cap, device=dev, dtype=torch.int64)
    block = torch.zeros(cap, W, device=dev, dtype=torch.float32)
    if ids.numel():
        id_block[: ids.numel()] = ids.to(torch.int64)
        block[: ids.numel()] = rows.to(torch.float32)
    id_blocks = [torch.empty_like(id_block) for _ in range(world)]
    blocks = [torch.empty_like(block) for _ in range(world)]
    dist.all_gather(id_blocks, id_block, group=group)
    dist.all_gather(blocks, block, group=group)
    all_ids = torch.cat([b[:c] for b, c in zip(id_blocks, counts)], 0)
    all_rows = torch.cat([b[:c] for b, c in zip(blocks, counts)], 0)
    order = torch.argsort(all_ids)
    return all_ids[order], all_rows[order]


def _with_key(batch, key):
    """A shallow copy of a B = 1 batch that carries ``complex_keys = [key]`` (the caller's batch is not touched)."""
    out = type(batch)(batch)
    out["complex_keys"] = [int(key)]
    return out


def _with_mask(batch, key, mask):
    """``_with_key`` plus the rows partial repacking keeps (``fixed_mask``, [1, L]; ``batch.pack`` carries both)."""
    out = _with_key(batch, key)
    out["complex_key"] = int(key)
    out["fixed_mask"] = (torch.as_tensor(mask).to(batch["X"].device) != 0).reshape(1, -1)
    return out


def sample_sharded(model, complexes, use_proximal=False, group=None, init_chi=None, max_rows=200_000, lengths=None,
                   rank=None, world=None, packed_proximal=True, seed=None, fixed_masks=None):
    """Run the sampling path on this rank's share of ``complexes`` (list of B = 1 batches already on the rank's device)
    and gather every complex's metric row on every rank.  With ``lengths`` (the residue counts of ALL complexes, known to
    every rank) ``complexes`` may be a dict {complex id: batch} that holds only this rank's share -- a rank need not build
    the other ranks' inputs.  ``rank`` / ``world`` override the process group's (a single process rehearsing the shards of
    an N-rank job one after the other; the gather then only orders the local rows).

    The shard is sampled as ragged PACKED batches (``batch.pack``: no padding rows are launched; complexes shorter than 32
    residues go alone because K = min(32, L)), at most ``max_rows`` residues per batch.  The proximal stage, which the
    reference defines for one complex at a time (optimize.py:27), runs on the packed group as well (``packed_proximal``: one
    ``proximal_optimizer_packed`` call per group, every complex with its own clash mask, normalisers -- its padded
    ``max_size``, as the per-complex call divides --, losses and accept rule: the same bits); ``packed_proximal=False`` keeps
    one ``proximal_optimizer`` call per complex.  The metrics of the proximal branch run per complex.
    ``init_chi`` (optional, {complex id: [1, L, 4]}) injects the initial noised angles instead of drawing them.
    ``seed`` (optional): all noise comes from the device generator (``TDiffusionModule.sampling(seed=...)``) and the key of every
    complex is its global id, in packed groups and single-complex groups alike: a complex's sample does not depend on
    ``world``, ``rank``, ``max_rows`` or what it was grouped with.  ``seed`` and ``init_chi`` exclude each other.
    ``fixed_masks`` (optional, {complex id: [1, L] mask} or a list, 1 = keep; needs ``seed``): partial repacking -- every group goes
    through ``TDiffusionModule.repack`` with the global ids as keys, the kept rows come out as the complex's ``SC_D`` bit for bit,
    and the proximal stage is the pinned one (one call per packed group with the padded sizes, or one per complex), with the same
    independence of ``world``, ``rank``, ``max_rows`` and grouping.
    Complexes that carry obstacle atoms (``protein_to_batch(..., obstacles=...)``) are refused with ``ValueError``.
    Returns (chi per local complex id, ids_all, rows_all)."""
    from .batch import group_rows, has_obstacles, pack, pad_rows, unpack
    from .functional import proximal_optimizer, proximal_optimizer_packed
    if any(has_obstacles(c) for c in (complexes.values() if isinstance(complexes, dict) else complexes)):
        raise ValueError("sample_sharded does not support complexes with obstacle atoms (DESIGN.md section 19: out of scope)")
    if seed is not None and init_chi is not None:
        raise ValueError("seed and init_chi exclude each other: a seeded run draws its own initial angles")
    if fixed_masks is not None and seed is None:
        raise ValueError("fixed_masks needs seed: partial repacking draws its noise from the seeded device generator")
    if rank is None:
        rank = dist.get_rank(group) if dist.is_initialized() else 0
    if world is None:
        world = dist.get_world_size(group) if dist.is_initialized() else 1
    if lengths is None:
        lengths = [int(c["max_size"]) for c in complexes]
    mine = shard_complexes(lengths, world)[rank]
    cfg = model.hparams.sample_cfg
    true_counts = (torch.stack([(complexes[i]["residue_mask"] > 0).sum() for i in mine]).tolist() if mine else [])   # one read-back
    mine_sizes = [int(complexes[i]["max_size"]) for i in mine]
    # K = min(32, L) is a property of the batch (encoder.py:115): a complex that is shorter than 32 rows once its trailing
    # padding is dropped goes through the plain B = 1 path with its own tensors, as the reference would run it
    alone = [n_true < 32 or n < 32 for n_true, n in zip(true_counts, mine_sizes)]
    groups = [[mine[k] for k in g] for g in group_rows(mine_sizes, alone, max_rows)]
    chis, row_of, proxed = {}, {}, set()
    cfg_prox = (cfg.violation_tolerance_factor, cfg.clash_overlap_tolerance, cfg.lamda, cfg.num_steps)
    for grp in groups:
        if fixed_masks is not None:       # partial repacking: the pinned sampler, then the pinned proximal stage
            if len(grp) == 1:
                i = grp[0]
                chis[i] = model.repack(_with_mask(complexes[i], i, fixed_masks[i]), seed=seed, use_proximal=use_proximal)
                proxed.add(i)
                continue
            pb = pack([_with_mask(complexes[i], i, fixed_masks[i]) for i in grp])
            sizes = [int(complexes[i]["max_size"]) for i in grp]
            out = model.repack(pb, seed=seed, use_proximal=use_proximal and packed_proximal, norm_rows=sizes)
            if not use_proximal:
                for i, row in zip(grp, packed_metric_rows(model, pb, out, sizes)):
                    row_of[i] = row
            elif packed_proximal:
                proxed.update(grp)
            for i, chi in zip(grp, unpack(pb, out)):
                chis[i] = pad_rows(chi, int(complexes[i]["max_size"]), fresh=True)
            continue
        if len(grp) == 1:
            i = grp[0]
            if init_chi is not None:
                chis[i] = model.sample_from(complexes[i], init_chi[i].to(model.device))
            elif seed is not None:
                chis[i] = model.sampling(_with_key(complexes[i], i), seed=seed)
            else:
                chis[i] = model.sampling(complexes[i])
            continue
        pb = pack([complexes[i] for i in grp])
        if init_chi is not None:
            offs = pb["seg_offsets_host"]
            x0 = torch.cat([init_chi[i][:, :b - a] for i, a, b in zip(grp, offs[:-1], offs[1:])], 1).to(model.device)
            out = model.sample_from(pb, x0)
        elif seed is not None:
            pb["complex_keys"] = [int(i) for i in grp]
            out = model.sampling(pb, seed=seed)
        else:
            out = model.sampling(pb)
        if not use_proximal:          # the metrics of the whole group in one go (the proximal stage changes the angles first)
            for i, row in zip(grp, packed_metric_rows(model, pb, out, [int(complexes[i]["max_size"]) for i in grp])):
                row_of[i] = row
        elif packed_proximal:         # the proximal stage of the whole group in one go, each complex divided by its padded size
            out = proximal_optimizer_packed(pb, out, cfg.violation_tolerance_factor, cfg.clash_overlap_tolerance, cfg.lamda,
                                            cfg.num_steps, norm_rows=[int(complexes[i]["max_size"]) for i in grp])[2]
            proxed.update(grp)
        for i, chi in zip(grp, unpack(pb, out)):
            chis[i] = pad_rows(chi, int(complexes[i]["max_size"]))
    rows = []
    for i in mine:
        if use_proximal and i not in proxed and fixed_masks is not None:      # the per-complex pinned call, accept rule on the device
            chis[i] = proximal_optimizer_packed(complexes[i], chis[i], *cfg_prox, fixed_mask=fixed_masks[i])[2]
        elif use_proximal and i not in proxed:
            lst, losses = proximal_optimizer(complexes[i], chis[i], cfg.violation_tolerance_factor,
                                             cfg.clash_overlap_tolerance, cfg.lamda, cfg.num_steps)
            if losses[-1] < losses[0]:
                chis[i] = lst[-1]
        rows.append(row_of[i] if i in row_of else metrics_to_row(model.analyze_samples(complexes[i], chis[i])))
    dev = model.device
    ids = torch.tensor(mine, device=dev, dtype=torch.int64)
    rows_t = torch.stack(rows).to(dev) if rows else torch.zeros(0, len(METRIC_KEYS), device=dev)
    ids_all, rows_all = gather_metric_rows(ids, rows_t, group)
    return chis, ids_all, rows_all
