"""Element-wise attention tests on the GPU: every attention kernel, forward and backward, against the float64
reference and the derived bounds of tests/attn_exact_util.py (checked on the CPU by tests/test_attn_exact_ref.py).

* the tiled kernels of csrc/flash_attn.hip with one and with two 16-row blocks per wave (``blocks`` 1 / 2: both
  template variants of the forward, dQ and dK/dV kernels), at every sequence length around the 16 / 64 / 128-row tile
  edges, grouped-query layouts, head mask and general splice, padded / packed / minimally aligned buffers;
* the MFMA short-sequence kernel (csrc/attn_mfma.hip, S <= 16) with its paired and spec entry points;
* the VALU kernel (csrc/kernels.hip, S <= 64) up to its LDS limit, and the refusal beyond it.

A case passes only with no element outside its bound, no padding element touched and (flash) a log-sum-exp within
2^-18 of the reference.

Measured on an MI355X: 577 cases, 577 passed, none skipped, 13.5 s for the module; every case below 0.1 s but the two
that pay a one-time initialisation (the first launch, 1.1 s, and the first fp32 einsum of the fallback case, 1.1 s).
Launches with 64 to 160 KiB of dynamic LDS (the VALU kernel at S = 64, dh = 96 / 128) are accepted as they are.  As a
check of the module itself, a forward whose second 16-row block admits key i + 1 under the causal mask -- a fault only
the two-block variants can have -- failed all 32 causal ``blocks`` = 2 cases of the bound and count families from
S = 63 on and none of the ``blocks`` = 1 cases.
"""
import math

import pytest
import torch

import attn_exact_util as X
from test_attn_exact_ref import FLASH_DH, FLASH_S, LAYOUTS, MFMA_DH, MFMA_S, VALU_DH, VALU_S, kernel_scale

pytestmark = pytest.mark.gpu

dev = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
FAMILIES = ["bound", "selector", "count"]


@pytest.fixture(scope="module")
def K():
    from iit_amd.ops import hip_kernels
    hip_kernels.lib()
    return hip_kernels


def _cuda(d: dict) -> dict:
    return {n: (t.to(dev) if isinstance(t, torch.Tensor) else t) for n, t in d.items()}


def _report(bad: dict):
    return {n: int(m.sum()) for n, m in bad.items() if int(m.sum())}


def _operand_sets(family, B, S, Hq, Hkv, dh, causal, scale, seed, sel=None, src=None):
    """[(name, operands on the GPU, check(got) -> masks)] of one family."""
    out = []
    if family == "bound":
        c = _cuda(X.bound_case(B, S, Hq, Hkv, dh, seed))
        ref = X.reference(c["q"], c["k"], c["v"], c["do"], causal, scale, sel, src)
        out.append(("bound", c, lambda got, ref=ref: X.check_bound(got, ref)))
    elif family == "selector":
        c = X.selector_case(B, S, Hq, Hkv, dh, causal, scale, seed, None if sel is None else sel.cpu(),
                            None if src is None else src.cpu())
        want = _cuda(c["want"])
        out.append(("selector", _cuda(c), lambda got, want=want: X.check_selector(got, want)))
    else:
        for name, c, count in X.count_cases(B, S, Hq, Hkv, dh, causal, seed):
            c = _cuda(c)
            ref = X.reference(c["q"], c["k"], c["v"], c["do"], causal, scale, sel, src)
            out.append((name, c, lambda got, ref=ref, count=count.to(dev): X.check_count(got, ref, count)))
    return out


# ================================================================================================ flash
def run_flash(K, c, causal, scale, blocks, layout, head_mask=0, spec=None, src=None):
    """Forward + backward of csrc/flash_attn.hip on padded buffers; returns the five outputs (views into their
    sentinel-prefilled buffers) after checking that no padding element changed."""
    B, S, Hq, dh = c["q"].shape
    Hkv = c["k"].shape[2]
    if layout == "packed":
        (q, k, v), _ = X.embed_packed(c["q"], c["k"], c["v"], device=dev)
        lay = "padded"
    else:
        q, k, v = (X.embed(c[n], layout, device=dev)[0] for n in ("q", "k", "v"))
        lay = layout
    do, _ = X.embed(c["do"], lay, device=dev)
    z, zbuf, zpre = X.out_like((B, S, Hq, dh), lay, BF16, dev)
    lse, lbuf, lpre = X.out_like((B, Hq, S), lay, F32, dev)
    dd, dbuf, dpre = X.out_like((B, Hq, S), lay, F32, dev)
    if layout == "packed":  # gradients into the three views of one packed buffer, as the model's backward does
        gbuf = torch.full((B, S + 2, 3, Hq, dh), X.BF16_FILL, dtype=BF16, device=dev)
        gpre = gbuf.clone()
        dq, dk, dv = (gbuf[:, :S, n] for n in range(3))
        gchecks = [((dq, dk, dv), gbuf, gpre)]
    else:  # strides at the 8-byte minimum of the gradient stores
        gs = [X.out_like((B, S, h, dh), lay, BF16, dev, align=4) for h in (Hq, Hkv, Hkv)]
        dq, dk, dv = (g[0] for g in gs)
        gchecks = [(g[0], g[1], g[2]) for g in gs]
    K.flash_fwd(q, k, v, z, lse, src, head_mask, scale, causal, spec=spec, blocks=blocks)
    K.flash_bwd(q, k, v, z, do, lse, dd, dq, dk, dv, head_mask, scale, causal, spec=spec, blocks=blocks)
    torch.cuda.synchronize()
    for views, buf, pre in [(z, zbuf, zpre), (lse, lbuf, lpre), (dd, dbuf, dpre)] + gchecks:
        assert X.padding_touched(views, buf, pre) == 0
    return {"z": z, "lse": lse, "dq": dq, "dk": dk, "dv": dv}


def _layout(si, dh, causal, Hq, Hkv):
    lay = ("contig", "padded", "packed")[(si + dh // 64 + int(causal)) % 3]
    return "padded" if lay == "packed" and Hq != Hkv else lay


def _plan_matches(K, B, S, Hq, Hkv, dh, blocks):
    """The launch plan for a forced ``blocks``: the count reaches the grid arithmetic of all three launches."""
    p = K.flash_plan(B, S, Hq, Hkv, dh, blocks)
    nkv = 1 if dh == 128 else blocks
    assert p == {"nb_q": blocks, "nb_kv": nkv, "grid_q": -(-S // (64 * blocks)), "grid_kv": -(-S // (64 * nkv))}, p


@pytest.mark.parametrize("blocks", [1, 2])
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("dh", FLASH_DH)
@pytest.mark.parametrize("S", FLASH_S)
def test_flash(K, S, dh, causal, family, blocks):
    si = FLASH_S.index(S)
    Hq, Hkv = LAYOUTS[si % 3]
    B = 2 + si % 2
    scale = kernel_scale(dh)
    _plan_matches(K, B, S, Hq, Hkv, dh, blocks)
    for name, c, check in _operand_sets(family, B, S, Hq, Hkv, dh, causal, scale, seed=S + dh):
        got = run_flash(K, c, causal, scale, blocks, _layout(si, dh, causal, Hq, Hkv))
        bad = check(got)
        assert X.n_bad(bad) == 0, (name, _report(bad))


SPLICES = ["head_mask", "positions_heads", "dims", "batch_pos", "broadcast_src"]


@pytest.mark.parametrize("blocks", [1, 2])
@pytest.mark.parametrize("family", ["bound", "selector"])
@pytest.mark.parametrize("which", SPLICES)
@pytest.mark.parametrize("S,dh", [(129, 64), (65, 128)])
def test_flash_splice(K, S, dh, which, family, blocks):
    """Head mask and general splice spec (the index kinds of tests/test_flash_attn.py's splice test plus a broadcast
    source): spliced elements equal the source bitwise (their bound is 0) and carry exactly zero gradient (the
    reference's dO is zero there, so dq / dk / dv have to match the reference of the masked dO)."""
    from iit_amd.core.index import Ix
    from iit_amd.ops.splice import patch_spec
    B, Hq, Hkv, causal = 3, 6, 2, True
    scale = kernel_scale(dh)
    g = torch.Generator().manual_seed(11)
    srcv = X.bf16_exact(torch.randint(-8, 9, (B, S, Hq, dh), generator=g).double() / 4)
    if which == "broadcast_src":
        srcv = srcv[:1]
    src, _ = X.embed(srcv, "padded" if which != "broadcast_src" else "contig", device=dev)
    if which == "head_mask":
        mask, spec = 0b100010, None
        sel = X.head_mask_sel((B, S, Hq, dh), mask, dev)
    else:
        idx = {"positions_heads": Ix[None, 5:70, [1, 4], None], "dims": Ix[None, None, 3, 16:50],
               "batch_pos": Ix[[0, 2], -1, None, None], "broadcast_src": Ix[None, 10:20, 2:4, None]}[which]
        mask, spec = 0, patch_spec(idx, (B, S, Hq, dh), src)
        assert spec is not None
        sel = torch.zeros(B, S, Hq, dh, dtype=torch.bool, device=dev)
        sel[idx.as_index] = True
    for name, c, check in _operand_sets(family, B, S, Hq, Hkv, dh, causal, scale, S + dh, sel, srcv.to(dev)):
        got = run_flash(K, c, causal, scale, blocks, "padded", mask, spec, src)
        bad = check(got)
        assert X.n_bad(bad) == 0, (name, _report(bad))
        assert torch.equal(got["z"][sel], src.expand(B, S, Hq, dh)[sel])
        if which == "head_mask":
            assert int((got["dq"][:, :, [1, 5]] != 0).sum()) == 0


def test_flash_policy_picks_two_blocks_and_launches_repeat_bitwise(K):
    """A shape at which the unforced policy (``blocks`` 0) itself takes two blocks per wave for all three kernels --
    ceil(S / 128) * heads * B = 2 * 16 * 16 = 512 -- under the bounds, equal bit for bit to the forced two-block
    launch; a repeat of each launch into fresh buffers gives the same bits (no atomics, no uninitialised reads)."""
    B, S, H, dh, causal = 16, 130, 16, 64, True
    assert K.flash_plan(B, S, H, H, dh, 0) == {"nb_q": 2, "nb_kv": 2, "grid_q": 2, "grid_kv": 2}
    assert K.flash_plan(B, S, H, H, dh, 1) == {"nb_q": 1, "nb_kv": 1, "grid_q": 3, "grid_kv": 3}
    assert K.flash_plan(15, S, H, H, dh, 0)["nb_q"] == 1  # 480 workgroups: below the threshold
    scale = kernel_scale(dh)
    (_, c, check), = _operand_sets("bound", B, S, H, H, dh, causal, scale, seed=5)
    got0 = run_flash(K, c, causal, scale, 0, "padded")
    bad = check(got0)
    assert X.n_bad(bad) == 0, _report(bad)
    for blocks, first in ((2, got0), (1, None)):
        for _ in range(2):
            got = run_flash(K, c, causal, scale, blocks, "padded")
            if first is None:
                first = got
                assert X.n_bad(check(got)) == 0
            for n in X.OUTPUTS:
                assert torch.equal(X.bits(got[n]), X.bits(first[n])), (blocks, n)


def test_flash_blocks_argument_is_checked(K):
    """``blocks`` outside {0, 1, 2} is refused by the wrappers and by the exports (before any launch); dK/dV at
    dh 128 stays at one block whatever is asked, and the call succeeds (test_flash runs it)."""
    with pytest.raises(ValueError):
        K.flash_plan(2, 129, 4, 2, 64, 3)
    q = torch.zeros(1, 16, 1, 64, dtype=BF16, device=dev)
    lse = torch.zeros(1, 1, 16, device=dev)
    with pytest.raises(ValueError):
        K.flash_fwd(q, q, q, q.clone(), lse, None, 0, 1.0, True, blocks=3)
    with pytest.raises(ValueError):
        K.flash_bwd(q, q, q, q, q, lse, lse.clone(), q.clone(), q.clone(), q.clone(), 0, 1.0, True, blocks=-1)
    out = (K.c_int * 4)()
    import ctypes
    assert K.lib().iit_flash_plan(2, 129, 4, 2, 64, 3, ctypes.cast(out, K.c_void_p)) != 0
    assert K.flash_plan(2, 129, 4, 2, 128, 2) == {"nb_q": 2, "nb_kv": 1, "grid_q": 2, "grid_kv": 3}


# ================================================================================================ short kernels
def _rows(t, B, S):
    return t.reshape(B * S, -1)


def run_small(K, c, causal, scale, mask=0, src=None, pad=8, backward=True):
    """attn_small_fwd / attn_small_bwd (MFMA for S <= 16 and dh in 32 / 64 / 96 / 128, else VALU) on a packed qkv
    [B*S, 3*H*dh + pad] with NaN padding columns and rows; outputs into sentinel-prefilled padded buffers."""
    B, S, H, dh = c["q"].shape
    HD = H * dh
    T = B * S

    def buf(width, fill, data=None):
        b = torch.full((T + 2, width + pad), fill, dtype=BF16, device=dev)
        if data is not None:
            b[:T, :width] = data.to(BF16)
        return b

    qkv = buf(3 * HD, X.NAN, torch.cat([_rows(c[n], B, S) for n in ("q", "k", "v")], 1))
    dz = buf(HD, X.NAN, _rows(c["do"], B, S))
    zs = None if src is None else buf(HD, X.NAN, _rows(src, B, S))
    z, dqkv = buf(HD, X.BF16_FILL), buf(3 * HD, X.BF16_FILL)
    zpre, gpre = z.clone(), dqkv.clone()
    lse = torch.full((B * H * S + 16,), X.NAN, device=dev)
    K.attn_small_fwd(qkv, z, lse, zs, mask, B, S, H, dh, 3 * HD + pad, HD + pad, HD + pad, scale, causal)
    if backward:
        K.attn_small_bwd(qkv, dz, lse, dqkv, mask, B, S, H, dh, 3 * HD + pad, HD + pad, scale, causal)
    torch.cuda.synchronize()
    return _small_outputs(z, zpre, dqkv, gpre, lse, B, S, H, dh, backward)


def _small_outputs(z, zpre, dqkv, gpre, lse, B, S, H, dh, backward=True, Bz=None):
    """The five outputs of ``B`` sequences as [B,S,H,dh] / [B,H,S] views, after checking that the padding of the
    buffers kept its bits (``Bz``: sequences the forward wrote, when more than ``B``)."""
    HD, T = H * dh, B * S
    Bz = Bz or B
    for b, pre, w, rows in ((z, zpre, HD, Bz * S), (dqkv, gpre, 3 * HD, T)):
        pre = pre.clone()
        if b is dqkv and not backward:
            continue
        pre[:rows, :w] = b[:rows, :w]
        assert torch.equal(X.bits(b), X.bits(pre)), "padding touched"
    assert bool(torch.isnan(lse[Bz * H * S:]).all())
    g = dqkv[:T, :3 * HD].reshape(B, S, 3, H, dh)
    return {"z": z[:T, :HD].reshape(B, S, H, dh), "lse": lse[:B * H * S].view(B, H, S), "dq": g[:, :, 0],
            "dk": g[:, :, 1], "dv": g[:, :, 2]}


def _small_case(K, family, B, S, H, dh, causal, mask, pad=8, backward=True):
    scale = kernel_scale(dh)
    sel = X.head_mask_sel((B, S, H, dh), mask, dev) if mask else None
    g = torch.Generator().manual_seed(13)
    src = X.bf16_exact(torch.randint(-8, 9, (B, S, H, dh), generator=g).double() / 4).to(dev) if mask else None
    for name, c, check in _operand_sets(family, B, S, H, H, dh, causal, scale, S + dh, sel, src):
        got = run_small(K, c, causal, scale, mask, src, pad, backward)
        bad = check(got)
        if not backward:
            bad = {n: m for n, m in bad.items() if n in ("z", "lse", "count")}
        assert X.n_bad(bad) == 0, (name, _report(bad))
        if mask:
            assert torch.equal(got["z"][sel].double(), src[sel])


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("dh", MFMA_DH)
@pytest.mark.parametrize("S", MFMA_S)
def test_mfma_short(K, S, dh, causal, family):
    """csrc/attn_mfma.hip: B * H a multiple of the four waves of a workgroup (2 x 4) and not (3 x 3); the head mask
    alternates with the plain launch."""
    si = MFMA_S.index(S)
    B, H = ((3, 3), (2, 4))[(si + dh // 32) % 2]
    mask = 0b10 if (si + int(causal)) % 2 else 0
    assert K._mfma_attn(S, dh)
    _small_case(K, family, B, S, H, dh, causal, mask)


# every (S, dh) of the two lists that the MFMA kernel does not take (S = 1 with dh 96 is its own)
VALU_CASES = [(S, dh) for S in VALU_S for dh in VALU_DH if not (S <= 16 and dh in MFMA_DH)]


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("S,dh", VALU_CASES)
def test_valu_short(K, S, dh, family):
    """csrc/kernels.hip attn_small: S up to 64 with head dims the MFMA kernel does not take (16, 24) and the largest
    the dispatcher sends there at S = 64 (96: 132,608 B of dynamic LDS for the backward); odd leading dimensions."""
    si = VALU_S.index(S)
    assert not K._mfma_attn(S, dh)
    causal = bool((si + dh // 8) % 2)
    mask = 0b01 if (si + dh) % 2 else 0
    _small_case(K, family, 2, S, 3, dh, causal, mask, pad=3)


@pytest.mark.parametrize("family", FAMILIES)
def test_valu_forward_at_the_lds_limit(K, family):
    """S = 64, dh = 128: the forward's 115,712 B of LDS fit, so it runs; the backward's 165,376 B do not."""
    _small_case(K, family, 2, 64, 2, 128, True, 0b10, pad=3, backward=False)


def test_oversized_lds_requests_are_refused(K):
    """Both exports return an error (no launch) for a request they cannot be given: the backward at S = 64,
    dh = 128 (165,376 B > 160 KiB) and anything past dh 128, where the forward's request grows beyond it too."""
    B, S, H = 1, 64, 1
    for dh, fwd_ok in ((128, True), (192, False)):
        HD = H * dh
        qkv = torch.zeros(B * S, 3 * HD, dtype=BF16, device=dev)
        z = torch.zeros(B * S, HD, dtype=BF16, device=dev)
        lse = torch.zeros(B * H * S, device=dev)
        assert K.attn_small_lds(S, dh, True) > K.ATTN_SMALL_LDS_MAX
        args = (B, S, H, dh, 3 * HD, HD)
        rc = K.lib().iit_attn_small_fwd(qkv.data_ptr(), z.data_ptr(), lse.data_ptr(), None, 0, *args, HD, 1.0, 1,
                                        K._stream())
        assert (rc == 0) == fwd_ok
        rc = K.lib().iit_attn_small_bwd(qkv.data_ptr(), z.data_ptr(), lse.data_ptr(), qkv.clone().data_ptr(), 0, *args,
                                        1.0, 1, K._stream())
        assert rc != 0
        torch.cuda.synchronize()
    with pytest.raises(RuntimeError):
        K.attn_small_bwd(qkv, z, lse, qkv.clone(), 0, B, S, H, 128, 3 * 128, 128, 1.0, True)


def test_hipops_attention_falls_back_at_the_lds_limit(K, monkeypatch):
    """HipOps.attention with the flash kernels switched off at S = 64, dh = 128 takes the torch path (the VALU
    backward would be refused) and returns correct z and gradients.  The operands are fp32 tensors of bf16-exact
    values, so the fallback computes in fp32 and has to stay inside the kernels' bounds."""
    from iit_amd.ops import hip_ops
    from iit_amd.ops.torch_ops import TorchOps
    monkeypatch.setenv("IIT_FLASH", "0")
    monkeypatch.setattr(K, "attn_small_fwd", lambda *a, **k: pytest.fail("the short-sequence kernel was launched"))
    ops = hip_ops.HipOps.__new__(hip_ops.HipOps)
    TorchOps.__init__(ops, BF16)
    B, S, H, dh = 2, 64, 2, 128
    c = _cuda(X.bound_case(B, S, H, H, dh, seed=9))
    ref = X.reference(c["q"], c["k"], c["v"], c["do"], True, 1 / math.sqrt(dh))
    q, k, v = (c[n].float().requires_grad_() for n in ("q", "k", "v"))
    z = ops.attention(q, k, v, True, math.sqrt(dh))
    z.backward(c["do"].float())
    got = {"z": z.detach(), "lse": ref["lse"], "dq": q.grad, "dk": k.grad, "dv": v.grad}
    bad = X.check_bound(got, ref)
    assert X.n_bad(bad) == 0, _report(bad)


# ------------------------------------------------------------------------------------------------ paired / spec entries
def _pair_buffers(c, B2, S, H, dh):
    HD, T = H * dh, B2 * S
    qkv = torch.full((T + 2, 3 * HD + 8), X.NAN, dtype=BF16, device=dev)
    qkv[:T, :3 * HD] = torch.cat([_rows(c[n], B2, S) for n in ("q", "k", "v")], 1).to(BF16)
    z = torch.full((T + 2, HD + 8), X.BF16_FILL, dtype=BF16, device=dev)
    lse = torch.full((B2 * H * S + 16,), X.NAN, device=dev)
    return qkv, z, lse


def _base_backward(K, c, qkv, lse, Bp, S, H, dh, scale, causal, mask=0, spec=None):
    HD, T = H * dh, Bp * S
    dz = torch.full((T + 2, HD + 8), X.NAN, dtype=BF16, device=dev)
    dz[:T, :HD] = _rows(c["do"][:Bp], Bp, S).to(BF16)
    dqkv = torch.full((T + 2, 3 * HD + 8), X.BF16_FILL, dtype=BF16, device=dev)
    gpre = dqkv.clone()
    if spec is None:
        K.attn_small_bwd(qkv, dz, lse, dqkv, mask, Bp, S, H, dh, 3 * HD + 8, HD + 8, scale, causal)
    else:
        K.attn_bwd_spec(qkv, dz, lse, dqkv, Bp, S, H, dh, 3 * HD + 8, HD + 8, scale, causal, spec.ptr)
    torch.cuda.synchronize()
    return dqkv, gpre


@pytest.mark.parametrize("family", ["bound", "selector"])
@pytest.mark.parametrize("which", ["pair_mask", "positions", "head_list", "partial_chunk"])
@pytest.mark.parametrize("S,dh,causal", [(5, 32, True), (13, 96, False), (16, 64, True), (16, 128, True)])
def test_mfma_paired_entries(K, S, dh, causal, which, family):
    """attn_pair_fwd (``z2``, ``pair_seqs``, ``pair_mask``) and attn_pair_fwd_spec + attn_bwd_spec at kernel level:
    2 * Bp sequences, the first Bp base rows, the rest source rows.  Every row's z is inside the bounds of its own
    attention; the selected elements of the base rows equal the source rows' stored z bit for bit and carry no
    gradient; the lse of every live head is checked."""
    from iit_amd.core.index import Ix
    from iit_amd.ops.splice import patch_spec
    Bp, H = 3, 3
    B2, HD = 2 * Bp, 3 * dh
    scale = kernel_scale(dh)
    (name, c, _), = _operand_sets(family, B2, S, H, H, dh, causal, scale, S + dh)
    qkv, z, lse = _pair_buffers(c, B2, S, H, dh)
    zpre = z.clone()
    spec = None
    if which == "pair_mask":
        mask = 0b101
        z2 = torch.full_like(z, X.BF16_FILL)
        K.attn_pair_fwd(qkv, z, lse, B2, S, H, dh, 3 * HD + 8, HD + 8, scale, causal, z2=z2, pair_seqs=Bp,
                        pair_mask=mask)
        sel = X.head_mask_sel((Bp, S, H, dh), mask, dev)
    else:
        idx = {"positions": Ix[None, 1:3, None, None], "head_list": Ix[None, None, [0, 2], None],
               "partial_chunk": Ix[None, None, 1, 3:13]}[which]
        mask = 0
        spec = patch_spec(idx, (Bp, S, H, dh))
        assert spec is not None
        K.attn_pair_fwd_spec(qkv, z, lse, B2, S, H, dh, 3 * HD + 8, HD + 8, scale, causal, Bp, spec.ptr)
        sel = torch.zeros(Bp, S, H, dh, dtype=torch.bool, device=dev)
        sel[idx.as_index] = True
    torch.cuda.synchronize()
    dqkv, gpre = _base_backward(K, c, qkv, lse, Bp, S, H, dh, scale, causal, mask, spec)
    got = _small_outputs(z, zpre, dqkv, gpre, lse, Bp, S, H, dh, Bz=B2)
    zall = z[:B2 * S, :HD].reshape(B2, S, H, dh)
    zsrc = zall[Bp:].double()
    base = {n: c[n][:Bp] for n in ("q", "k", "v", "do")}
    srcs = {n: c[n][Bp:] for n in ("q", "k", "v", "do")}
    if family == "bound":
        ref = X.reference(base["q"], base["k"], base["v"], base["do"], causal, scale, sel, zsrc)
        bad = X.check_bound(got, ref)
        sref = X.reference(srcs["q"], srcs["k"], srcs["v"], srcs["do"], causal, scale)
        bad["z_src"] = X.bad_bound(zall[Bp:], sref["z"], sref["tol_z"])
        bad["lse_src"] = X.bad_lse(lse[Bp * H * S:B2 * H * S].view(Bp, H, S), sref["lse"])
    else:
        full = X.selector_case(B2, S, H, H, dh, causal, scale, S + dh)  # the operands of ``c``: same seed
        assert torch.equal(full["q"].to(dev), c["q"])
        want = _cuda(X.selector_case(B2, S, H, H, dh, causal, scale, S + dh,
                                     torch.cat([sel, torch.zeros_like(sel)]).cpu(),
                                     torch.cat([full["want"]["z"][Bp:], full["want"]["z"][Bp:]]))["want"])
        got_all = dict(got, z=zall, lse=lse[:B2 * H * S].view(B2, H, S))
        bad = {n: X.bad_exact(got[n], want[n][:Bp]) for n in ("dq", "dk", "dv")}
        bad["z"] = X.bad_exact(got_all["z"], want["z"])
        bad["lse"] = X.bad_lse(got_all["lse"], want["lse"], want["live"])
    assert X.n_bad(bad) == 0, (name, _report(bad))
    assert torch.equal(zall[:Bp][sel], zall[Bp:][sel])
    if which == "pair_mask":  # z2: a second copy of every row a wave stored itself (not the mirrored base heads)
        z2all = z2[:B2 * S, :HD].reshape(B2, S, H, dh)
        own = torch.ones(B2, S, H, dh, dtype=torch.bool, device=dev)
        own[:Bp] = ~sel
        assert torch.equal(z2all[own], zall[own])
        assert bool((z2all[~own] == X.BF16_FILL).all())
        z2c = z2.clone()
        z2c[:B2 * S, :HD] = X.BF16_FILL
        assert bool((z2c == X.BF16_FILL).all()), "z2 padding touched"
