"""``iit_sparse_pair_f32`` (csrc/splice.hip), the fp32 sparse pair splice, against torch indexing: mode 0 copies the
selected elements of the source half of a ``[2T][ld]`` activation into the base half in place, mode 1 zeroes the
selected elements of a ``[T][ld]`` gradient; everything else keeps its bits.  T = 6 rows (``[2][3]``), 10 columns in
use at row pitches 12 (a gap of two floats per row) and 10 (none); a pitch of 8 is refused for ten columns and runs
with eight."""
import pytest
import torch

import attn_f32_pair_util as P

gpu = pytest.mark.gpu
dev = "cuda"
T, COLS = 6, P.SPARSE_SHAPE[2]


def _kernels():
    from iit_amd.ops import hip_kernels as K
    return K


def _spec(index, shape=P.SPARSE_SHAPE):
    from iit_amd.ops.splice import patch_spec
    return patch_spec(index, tuple(shape))


def _act(rows, ld, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(rows, ld, generator=g).to(dev)


def _bits(t):
    return t.contiguous().view(torch.int32)


@gpu
@pytest.mark.parametrize("ld", [8, 12])
@pytest.mark.parametrize("name", list(P.SPARSE_INDEXES))
def test_both_modes_against_torch_indexing(name, ld):
    """Ten columns in use at ``ld = 12`` (two floats of gap per row) and at the dense pitch 10.  A pitch of 8 cannot
    hold ten columns: that call is refused with nothing written, and the pitch runs with the 8 columns it holds."""
    K = _kernels()
    index = P.SPARSE_INDEXES[name]
    if ld < COLS:
        spec = _spec(index, P.SPARSE_SHAPE)
        act = _act(2 * T, ld, 1)
        before = act.clone()
        for mode in (0, 1):
            with pytest.raises(ValueError):
                K.sparse_pair_f32(act, T, ld, spec, mode)
        stream = torch.cuda.current_stream().cuda_stream
        assert K.lib().iit_sparse_pair_f32(act.data_ptr(), T, ld, spec.ptr, 0, stream) != 0
        torch.cuda.synchronize()
        assert torch.equal(_bits(act), _bits(before))
    cols = min(COLS, ld)
    shape = P.SPARSE_SHAPE[:2] + (cols,)
    spec = _spec(index, shape)
    mask = P.index_mask(index, shape).reshape(T, cols).to(dev)
    for pitch in sorted({ld, cols}):
        full = torch.zeros(T, pitch, dtype=torch.bool, device=dev)
        full[:, :cols] = mask
        act = _act(2 * T, pitch, 2)
        want = act.clone()
        want[:T][full] = act[T:][full]
        K.sparse_pair_f32(act, T, pitch, spec, 0)
        assert torch.equal(_bits(act), _bits(want)), (name, pitch, "copy")
        grad = _act(T, pitch, 3)
        want = grad.clone()
        want[full] = 0.0
        K.sparse_pair_f32(grad, T, pitch, spec, 1)
        assert torch.equal(_bits(grad), _bits(want)), (name, pitch, "zero")


@gpu
def test_empty_selection_is_a_no_op():
    K = _kernels()
    spec = _spec(P.SPARSE_INDEXES["empty"])
    act = _act(2 * T, 12, 4)
    before = act.clone()
    K.sparse_pair_f32(act, T, 12, spec, 0)
    K.sparse_pair_f32(act[:T], T, 12, spec, 1)
    torch.cuda.synchronize()
    assert torch.equal(_bits(act), _bits(before))


@gpu
def test_refusals_raise_before_any_launch():
    K = _kernels()
    spec = _spec(P.SPARSE_INDEXES["neurons"])
    act = _act(2 * T, 12, 5)
    before = act.clone()
    for args in ((act, T + 1, 12, spec, 0),            # the spec's rows are not T
                 (act, T, 12, None, 0),                # no spec
                 (act, T, 12, spec, 2),                # no such mode
                 (act.bfloat16(), T, 12, spec, 0),     # not fp32
                 (_act(T, 12, 6), T, 12, spec, 0),     # mode 0 needs both halves
                 (act.cpu(), T, 12, spec, 1)):
        with pytest.raises(ValueError):
            K.sparse_pair_f32(*args)
    torch.cuda.synchronize()
    assert torch.equal(_bits(act), _bits(before))
