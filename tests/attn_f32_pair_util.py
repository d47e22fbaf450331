"""Expected values of the paired fp32 attention forward (``iit_attn_f32_fwd_pair``), of its masked backward and of
the fp32 sparse pair splice, composed on the host from plain results.

A ``PatchSpec`` is a range table: per dimension up to 8 half-open ranges; an element is selected iff every coordinate
lies in one of its dimension's ranges.  :func:`selection_mask` evaluates that sentence literally, with no torch
indexing, so that tests/test_attn_f32_pair_ref.py can hold it against ``torch.zeros(shape, dtype=bool)[index] = True``
for every index the GPU tests use (:func:`attn_indexes`, :data:`SPARSE_INDEXES`).
"""
import torch

from iit_amd.core.index import Ix

# (B, S, H, dh): one tile with padded rows; two tiles, dh % 16 != 0 and the vector path inside a packed row; the
# largest shape; the head of the 6-layer IOI model
CASES = ((2, 5, 3, 4), (2, 17, 2, 20), (1, 64, 1, 64), (3, 16, 4, 16))


def case_id(c) -> str:
    return "B{}-S{}-H{}-dh{}".format(*c)


def attn_indexes(shape) -> dict:
    """name -> TorchIndex over ``hook_z`` of base shape ``(B, S, H, dh)``."""
    B, S, H, dh = shape
    return {
        "one head": Ix[:, :, H - 1],
        "head list": Ix[:, :, sorted({0, H - 1})],
        "positions": Ix[:, 1:max(2, S // 2)],
        "features cut chunks": Ix[:, :, :, 1:7],
        "batch subset": Ix[B - 1:B],
        "heads x positions": Ix[:, 2:5, sorted({0, H - 1})],
        "everything": Ix[:, :, :, :],
    }


# over mlp.hook_post of base shape (B, S, 10) with B S = 6 rows
SPARSE_SHAPE = (2, 3, 10)
SPARSE_INDEXES = {
    "neurons": Ix[:, :, 2:7],
    "position and neurons": Ix[:, 1, 3:],
    "batch": Ix[1:2],
    "position list": Ix[:, [0, 2]],
    "everything": Ix[:, :, :],
    "empty": Ix[:, :, 4:4],
}


def selection_mask(spec, shape) -> torch.Tensor:
    """The boolean selection of ``spec`` (a ``PatchSpec``: ``dims`` = ``(extent, [(lo, hi), ...], stride)`` per
    dimension, leading dimensions padded with extent 1) as a tensor of ``shape``."""
    dims = spec.dims
    assert len(dims) == 4
    lines = []
    for n, runs, _ in dims:
        assert len(runs) <= 8
        lines.append(torch.tensor([any(lo <= c < hi for lo, hi in runs) for c in range(n)], dtype=torch.bool))
    mask = lines[0][:, None, None, None] & lines[1][None, :, None, None] & lines[2][None, None, :, None] \
        & lines[3][None, None, None, :]
    return mask.reshape(tuple(shape))


def index_mask(index, shape) -> torch.Tensor:
    """What torch indexing selects: the reference for :func:`selection_mask`."""
    mask = torch.zeros(tuple(shape), dtype=torch.bool)
    mask[index.as_index] = True
    return mask


def paired_z(z_plain: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    """The paired forward's z from the plain forward's over the same 2B rows: the source half unchanged, the base
    half with the selected elements taken from the source half."""
    B = z_plain.shape[0] // 2
    return torch.cat([torch.where(mask, z_plain[B:], z_plain[:B]), z_plain[B:]])


def masked_dz(dz: torch.Tensor, mask: torch.Tensor, fill: float = 0.0) -> torch.Tensor:
    """dz with the selected elements replaced by ``fill`` (+0: what the masked backward computes with; NaN: what it
    must not read)."""
    return torch.where(mask, torch.full_like(dz, fill), dz)
