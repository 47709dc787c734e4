"""Resource sharding across the GPUs of one node.

Every (resource, rule) cell is independent given the replicated program and
namespace-label table (MatchesResourceDescription reads only the resource, its
namespace labels and the rule: pkg/engine/utils/match.go:168), so ranks take
contiguous row ranges of one logical corpus and evaluate them with no data-path
collective. After the evaluation two exchanges exist: the per-rule totals
(kpe_counts, R x 7 u64) that `kyverno apply` prints
(cmd/cli/kubectl-kyverno/processor/result.go:34-68), summed with one all-reduce, and,
for a caller that reports from one process (the CLI's table of results), the
verdict rows gathered to one rank with grouped point-to-point transfers
(gather_rows: one send per rank, all receives posted together on the root). On GPU ranks
gather_packed sends each rank's matrix straight from HBM, packed on the device to 3-bit
cells (kpe_pack_verdicts into a torch buffer, 8/3 fewer bytes than the byte matrix).
"""
from typing import Dict, List, Optional, Sequence, Tuple

COUNT_FIELDS = ("na", "pass", "fail", "warn", "error", "skip", "undecided")


def shard_range(total: int, rank: int, world: int) -> Tuple[int, int]:
    """Contiguous [first, first+n) rows of a `total`-row corpus owned by `rank`.
    The first `total % world` ranks take one extra row."""
    if world <= 0 or not 0 <= rank < world:
        raise ValueError(f"bad rank {rank} / world {world}")
    base, extra = divmod(total, world)
    first = rank * base + min(rank, extra)
    return first, base + (1 if rank < extra else 0)


def counts_to_rows(counts: Sequence[Dict[str, int]]) -> List[List[int]]:
    return [[int(c[f]) for f in COUNT_FIELDS] for c in counts]


def rows_to_counts(rows) -> List[Dict[str, int]]:
    return [dict(zip(COUNT_FIELDS, (int(x) for x in r))) for r in rows]


def merge_namespace_counts(parts):
    """One per-namespace table from the shards' tables: parts is a sequence of (names, counts)
    pairs, names = Corpus.namespaces of a shard and counts its (G_i, R, 6) table
    (Engine.namespace_counts / kyverno_amd.namespace_counts). Every shard numbers its groups
    itself, so the tables are merged by namespace name, not by id: host only, and an all-reduce
    does not apply. Returns (names, counts): the names in first-seen order and a (G, R, 6) uint64
    table (sums over shards can pass 32 bits)."""
    import numpy as np

    index: Dict[str, int] = {}
    names: List[str] = []
    tabs = []
    for part_names, counts in parts:
        k = np.asarray(counts)
        if k.ndim != 3 or k.shape[0] != len(part_names) or k.shape[2] != 6:
            raise ValueError("merge_namespace_counts: (names, (len(names), R, 6) counts) pairs")
        if tabs and k.shape[1] != tabs[0][1].shape[1]:
            raise ValueError("merge_namespace_counts: the shards' tables differ in their rule count")
        ids = []
        for nm in part_names:
            if nm not in index:
                index[nm] = len(names)
                names.append(nm)
            ids.append(index[nm])
        tabs.append((np.asarray(ids, dtype=np.int64), k))
    R = tabs[0][1].shape[1] if tabs else 0
    out = np.zeros((len(names), R, 6), dtype=np.uint64)
    for ids, k in tabs:
        np.add.at(out, ids, k.astype(np.uint64))
    return names, out


def allreduce_counts(counts: Sequence[Dict[str, int]], device=None) -> List[Dict[str, int]]:
    """Sum per-rule counters over the default process group (RCCL on GPU ranks,
    gloo on CPU). One R x 6 int64 tensor; identity when not initialised."""
    import torch
    import torch.distributed as dist

    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
        return [dict(c) for c in counts]
    t = torch.tensor(counts_to_rows(counts), dtype=torch.int64, device=device)
    dist.all_reduce(t)
    return rows_to_counts(t.cpu().tolist())


def max_over_ranks(seconds: float, device=None) -> float:
    """The job's time is the slowest rank's (bench.py contract)."""
    import torch
    import torch.distributed as dist

    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
        return seconds
    t = torch.tensor([seconds], dtype=torch.float64, device=device)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t.item())


def gather_rows(local, total: int, dst: int = 0, device=None):
    """Gather every rank's contiguous verdict rows (shard_range order) of an N x R uint8
    matrix to rank `dst`: each rank posts one send, the root posts all receives in one
    batch_isend_irecv group (RCCL point-to-point over xGMI on GPU ranks, gloo on CPU).
    Returns the total x R matrix on `dst`, None elsewhere; the local rows when not
    initialised or world_size == 1."""
    import numpy as np
    import torch
    import torch.distributed as dist

    local = np.ascontiguousarray(local, dtype=np.uint8)
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
        return local
    world, rank = dist.get_world_size(), dist.get_rank()
    R = local.shape[1] if local.ndim == 2 else 0
    first, n = shard_range(total, rank, world)
    if local.shape[0] != n:
        raise ValueError(f"rank {rank} holds {local.shape[0]} rows, its shard has {n}")
    if R == 0:  # every rank knows R (the replicated program): nobody exchanges anything
        return np.zeros((total, 0), dtype=np.uint8) if rank == dst else None
    out: Optional["torch.Tensor"] = None
    if rank == dst:
        out = torch.empty((total, R), dtype=torch.uint8, device=device)
        if n:
            out[first:first + n] = torch.from_numpy(local).to(device)
        recv = {r: out[f:f + m].view(-1) for r, (f, m) in ((r, shard_range(total, r, world)) for r in range(world))}
        _p2p_to_root({r: v for r, v in recv.items() if r != dst}, None, dst, device)
        return out.cpu().numpy()
    _p2p_to_root(None, torch.from_numpy(local).to(device).view(-1), dst, device)
    return None


def _p2p_to_root(recv, send, dst, device):
    """One batch_isend_irecv group joined by every rank: the root posts a receive per rank
    (`recv`: rank -> flat tensor), each other rank one send. A rank with nothing to send (an
    empty shard) sends a one-element placeholder, so no rank skips the group: RCCL requires
    every rank of the group in the first point-to-point call."""
    import torch
    import torch.distributed as dist

    ops = []
    if recv is not None:
        for r, t in recv.items():
            ops.append(dist.P2POp(dist.irecv, t if t.numel() else torch.empty(1, dtype=t.dtype, device=t.device), r))
    else:
        ops.append(dist.P2POp(dist.isend, send if send.numel() else torch.zeros(1, dtype=send.dtype, device=send.device), dst))
    if ops:
        for req in dist.batch_isend_irecv(ops):
            req.wait()


def gather_packed(engine, ps, corpus, total: int, dst: int = 0, device=None):
    """gather_rows for a matrix that stays on the device: the rank's verdicts are packed on its
    GPU (kpe_pack_verdicts, 3-bit cells) into a torch buffer and sent from there (RCCL over xGMI
    on GPU ranks; on `gloo`, `device` is the CPU and the packed words are copied to the host
    first). The root unpacks every rank's words (kpe_unpack_verdicts) into the total x R matrix.
    Returns it on `dst`, None elsewhere."""
    import numpy as np
    import torch
    import torch.distributed as dist

    from .engine import packed_words, unpack_verdicts

    R = ps.num_rules
    n = corpus.n
    words = packed_words(n * R)
    gpu = torch.empty(max(words, 1), dtype=torch.int32, device=torch.device("cuda", engine.device.ordinal))
    engine.pack_verdicts(ps, corpus, gpu.data_ptr(), words)
    buf = gpu if (device is not None and torch.device(device).type == "cuda") else gpu.cpu()
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
        return unpack_verdicts(buf[:words].cpu().numpy().view(np.uint32), n, R)
    world, rank = dist.get_world_size(), dist.get_rank()
    first, m = shard_range(total, rank, world)
    if m != n:
        raise ValueError(f"rank {rank} holds {n} rows, its shard has {m}")
    if R == 0:
        return np.zeros((total, 0), dtype=np.uint8) if rank == dst else None
    parts = {}
    if rank != dst:
        _p2p_to_root(None, buf[:words], dst, device)
        return None
    for r in range(world):
        f, mr = shard_range(total, r, world)
        parts[r] = buf if r == dst else torch.empty(packed_words(mr * R), dtype=torch.int32, device=buf.device)
    _p2p_to_root({r: t for r, t in parts.items() if r != dst}, None, dst, device)
    out = np.empty((total, R), dtype=np.uint8)
    for r in range(world):
        f, mr = shard_range(total, r, world)
        if mr and R:
            w = packed_words(mr * R)
            out[f:f + mr] = unpack_verdicts(parts[r][:w].cpu().numpy().view(np.uint32), mr, R)
    return out
