"""The host-side expectations of tests/attn_f32_pair_util.py, checked without a GPU: the selection a ``PatchSpec``
range table describes equals what torch indexing selects, for every index and shape the GPU tests of the paired fp32
attention kernels and of the fp32 sparse pair splice use."""
import pytest
import torch

import attn_f32_pair_util as P
from iit_amd.ops.splice import patch_spec


@pytest.mark.parametrize("c", P.CASES, ids=P.case_id)
def test_range_table_selects_what_torch_indexing_selects(c):
    for name, index in P.attn_indexes(c).items():
        spec = patch_spec(index, c)
        assert spec is not None and [d[0] for d in spec.dims] == list(c), name
        want = P.index_mask(index, c)
        assert torch.equal(P.selection_mask(spec, c), want), name
        assert want.any(), name  # every index selects something at every shape
    assert P.index_mask(P.attn_indexes(c)["everything"], c).all()


def test_some_index_cuts_a_four_float_chunk_at_every_shape():
    for c in P.CASES:
        m = P.index_mask(P.attn_indexes(c)["features cut chunks"], c)
        chunks = m.reshape(-1, c[3] // 4, 4).sum(-1)
        assert ((chunks > 0) & (chunks < 4)).any(), c


def test_sparse_indexes_over_a_padded_three_dimensional_shape():
    for name, index in P.SPARSE_INDEXES.items():
        spec = patch_spec(index, P.SPARSE_SHAPE)
        assert spec is not None and [d[0] for d in spec.dims] == [1, *P.SPARSE_SHAPE], name
        assert torch.equal(P.selection_mask(spec, P.SPARSE_SHAPE), P.index_mask(index, P.SPARSE_SHAPE)), name
    assert not P.index_mask(P.SPARSE_INDEXES["empty"], P.SPARSE_SHAPE).any()


def test_paired_z_and_masked_dz_compose_as_documented():
    z = torch.arange(2 * 2 * 3 * 2 * 4, dtype=torch.float32).reshape(4, 3, 2, 4)
    mask = P.index_mask(P.Ix[:, 1, :, 1:3], (2, 3, 2, 4))
    out = P.paired_z(z, mask)
    assert torch.equal(out[2:], z[2:])
    assert torch.equal(out[:2][mask], z[2:][mask]) and torch.equal(out[:2][~mask], z[:2][~mask])
    dz = P.masked_dz(z[:2] + 1, mask)
    assert (dz[mask] == 0).all() and torch.equal(dz[~mask], (z[:2] + 1)[~mask])
    assert P.masked_dz(z[:2], mask, float("nan"))[mask].isnan().all()
