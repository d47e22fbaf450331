"""Element-wise tests of the fused BatchNorm kernels of csrc/bn_nhwc.hip on the GPU -- ``iit_bn_fwd``, ``iit_bn_bwd``
and ``iit_bn_fwd_tiles`` called directly with sentinel-prefilled outputs and a fresh zeroed ``ws`` -- against the
float64 references and bounds of tests/bn_exact_util.py (proved on the CPU by tests/test_bn_exact_ref.py).

* ``test_bn_stats``: every channel width ``covered()`` admits (8, 16, 64, 512, 2048) with the row counts of
  ``bn_rows`` (1, rpi - 1, rpi, rpi + 1, 8 rpi + 1, 64 rpi + 3, 136 rpi - 5: idle thread groups, a full group, a second
  workgroup with one row, nine workgroups, seventeen), bf16 and fp32 activations, the atomic and the two-level
  reduction, every operand family, and the options (training / eval, residual, ReLU, momentum 0.1 / 1, a prefilled /
  null ``num_batches_tracked``, prefilled / null ``dw`` and ``db``) rotated over the cases.  After every call: ``save``,
  the running statistics, ``nbt``, ``y``, ``coef``, ``dw``, ``db``, ``dx`` and ``dres`` within their bounds, the
  accumulator and the ticket (the first 16 C + 1 words of ``ws``) all zero bits; a second call on the same ``ws`` meets
  the same bounds, and with the two-level reduction agrees with the first bit for bit.  No case depends on a bitwise
  outcome of the atomic reduction (the ``exact`` family is order-free by construction).
* ``test_bn_stats_grid_cap``: C = 512, M = 65,541 -- ``grid_for`` caps at 2048 workgroups and the first thread adds nine
  rows, the two-level partials fill ``BN_PART_MAX``.
* ``test_bn_splice``: splice-on-read with hand-built specs (two and three ranges per dimension, channel ranges that
  are no multiple of 8, the pivot row inside and outside the splice, NCHW / channels-last / batch-broadcast sources).
* ``test_bn_tiles``: ``bn_tile_finalize_kernel`` on records cut from an activation, T = 1 to 1000.
* ``test_conv_epilogue_records``: the records a convolution's epilogue writes against the same launch's own output.
* ``test_bn_refusals``: arguments the exports refuse return before any launch (csrc/bn_nhwc.hip: ``shape_ok``, the
  null ``rmean`` check, ``make_xsplice`` and the ``T R != M`` check all precede the first ``hipLaunchKernelGGL``), so
  the outputs keep their sentinel.

Measured on an MI355X: 57 cases, 57 passed, none skipped, 8.6 s for the module; the slowest ids are the two grid-cap
cases (0.9 s each: 33.6 M elements and their float64 reference on the device) and the first case (0.6 s, one-time
initialisation); every other id 0.2 s or less.  Worst observed error in units of its bound, over all cases: ``y`` 0.992
and ``dx`` 0.992 (the bf16 store takes nearly all of the bound), ``mean`` 0.996 and ``rm`` 0.926 (the ``exact`` and
``lowvar`` families, where the sums carry no error and the bound is the single rounding of ``p + dm`` -- half an ulp at
a mantissa just above 1; ``rm`` at momentum 1 is that mean), ``dw`` 0.987 and ``db`` 0.793 (the one rounding of the add
into the prefill where the sum itself is small), ``rstd`` 0.785, ``rv`` 0.756, ``coef`` 0.175; tile finalize: ``mean``
0.806, ``rm`` 0.693, ``rv`` 0.441, ``rstd`` 0.196; conv records: ``S1`` 0.013, ``S2`` 0.160 of the order-free bound
(twelve tile / split combinations accepted).  ``rstd`` of the eval mode stayed within the 2 E it is held to.  A library
with five in-bounds value defects (``hit`` widened to the whole channel group, the M / (M - 1) factor dropped at M = 2
in the atomic finalize, the tile cross term times 0.9995, ``>=`` in the pool's scan, ``k2`` times 1.0001) failed 68 of
the 98 cases of this module and tests/test_maxpool_exact.py: every statistics and splice id, the 14 tile ids with
T > 1 and 18 pool ids; the cases the defects do not reach passed (T = 1, the conv records, the refusals, the bf16
grid-cap ids, where 1e-4 of ``k2`` is below the bf16 store).
"""
import pytest
import torch

import bn_exact_util as X

pytestmark = pytest.mark.gpu

dev = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
DT = {"bf16": BF16, "f32": F32}
WORST = {}

# training, residual, relu, momentum, nbt prefill (None: a null pointer), dw / db given
OPTIONS = [(True, True, True, 0.1, 41, True), (True, False, True, 1.0, None, True),
           (False, True, False, 0.1, 41, False), (True, False, False, 0.1, 41, False),
           (True, True, True, 1.0, 41, True), (False, False, True, 0.1, None, True),
           (True, True, False, 1.0, None, True), (True, False, True, 0.1, 41, True)]


@pytest.fixture(scope="module")
def K():
    from iit_amd.ops import hip_kernels
    hip_kernels.lib()
    old = hip_kernels.CHECK_BOUNDS
    hip_kernels.CHECK_BOUNDS = True
    yield hip_kernels
    hip_kernels.CHECK_BOUNDS = old


def _reduction(monkeypatch, red: str) -> str:
    monkeypatch.delenv("IIT_DETERMINISTIC", raising=False)
    if red == "two":
        monkeypatch.setenv("IIT_BN_REDUCE", "two")
    else:
        monkeypatch.delenv("IIT_BN_REDUCE", raising=False)
    return red


def _count(bad: dict) -> dict:
    return {n: int(m.sum()) for n, m in bad.items() if int(m.sum())}


def _note(ref: dict, keys) -> None:
    for k, g in keys:
        r = X.worst(g, ref[k], ref["tol_" + k])
        WORST[k] = max(WORST.get(k, 0.0), r)


def _armed(ws: torch.Tensor, C: int) -> bool:
    """The accumulator (8 slots of 2 C floats) and the ticket: all zero bits."""
    return not bool(ws[:X.BN_SLOTS * 2 * C + 1].view(torch.int32).any())


def _fwd(K, x, res, pr, opt, ws, splice=None):
    training, _, relu, mom, nbt0, _ = opt
    M, C = x.shape
    got = {"y": X.filled((M, C), x.dtype, dev), "save": X.filled((2 * C,), F32, dev), "rm": pr["rm"].clone(),
           "rv": pr["rv"].clone()}
    nbt = None if nbt0 is None else torch.tensor(nbt0, dtype=torch.long, device=dev)
    kw = {} if splice is None else dict(src=splice[0], spec=splice[1], H=splice[2], W=splice[3])
    K.bn_fwd(x, res, got["y"], ws, got["rm"], got["rv"], pr["w"], pr["b"], M, C, X.BN_EPS, relu, training, got["save"],
             mom, nbt, **kw)
    got["nbt"] = None if nbt is None else int(nbt.item())
    return got


def _bwd(K, dy, fwd, x, pr, opt, ws, splice=None):
    training, has_res, relu, _, _, has_dw = opt
    M, C = x.shape
    got = {"coef": X.filled((2 * C,), F32, dev), "dx": X.filled((M, C), x.dtype, dev),
           "dres": X.filled((M, C), x.dtype, dev) if has_res else None,
           "dw": pr["dw0"].clone() if has_dw else None, "db": pr["db0"].clone() if has_dw else None}
    kw = {} if splice is None else dict(src=splice[0], spec=splice[1], H=splice[2], W=splice[3])
    K.bn_bwd(dy, fwd["y"] if relu else None, x, fwd["save"], pr["w"], ws, got["coef"], M, C, training, got["dx"],
             got["dres"], got["dw"], got["db"], **kw)
    return got


def _same_bits(a: dict, b: dict) -> bool:
    for k, v in a.items():
        if torch.is_tensor(v):
            if int(X.bad_bits(v, b[k]).sum()):
                return False
        elif v != b[k]:
            return False
    return True


def _run_case(K, x, xp, hit, res, dy, pr, opt, depth, exact, two, splice=None, tag=()):
    """Forward and backward twice on one ``ws``; every output checked after every call."""
    training, has_res, relu, mom, nbt0, has_dw = opt
    M, C = x.shape
    ws = torch.zeros(K.bn_ws_floats(C), dtype=F32, device=dev)
    ref = X.bn_fwd_ref(xp, res, pr["w"], pr["b"], pr["rm"], pr["rv"], nbt0, eps=X.BN_EPS, mom=mom, relu=relu,
                       training=training, depth=depth, exact=exact)
    runs = []
    for rep in range(2):
        fwd = _fwd(K, x, res, pr, opt, ws, splice)
        torch.cuda.synchronize()
        assert _armed(ws, C), (tag, rep, "forward left the accumulator or the ticket set")
        bad = _count(X.bn_fwd_check(fwd, ref))
        assert not bad, (tag, rep, "fwd", bad)
        _note(ref, [("mean", fwd["save"][:C]), ("rstd", fwd["save"][C:]), ("y", fwd["y"])]
              + ([("rm", fwd["rm"]), ("rv", fwd["rv"])] if training else []))
        bref = X.bn_bwd_ref(dy, fwd["y"] if relu else None, xp, hit, fwd["save"], pr["w"],
                            pr["dw0"] if has_dw else None, pr["db0"] if has_dw else None, training=training,
                            depth=depth, exact=exact)
        bwd = _bwd(K, dy, fwd, x, pr, opt, ws, splice)
        torch.cuda.synchronize()
        assert _armed(ws, C), (tag, rep, "backward left the accumulator or the ticket set")
        bad = _count(X.bn_bwd_check(bwd, bref))
        assert not bad, (tag, rep, "bwd", bad)
        _note(bref, [("coef", bwd["coef"]), ("dx", bwd["dx"])] + ([("dw", bwd["dw"]), ("db", bwd["db"])]
                                                                       if has_dw else []))
        runs.append((fwd, {k: v for k, v in bwd.items() if v is not None}))
    if two:
        assert _same_bits(runs[0][0], runs[1][0]) and _same_bits(runs[0][1], runs[1][1]), (tag, "two-level not bitwise")


def _dev(d: dict) -> dict:
    return {k: v.to(dev) for k, v in d.items()}


# ================================================================================================ statistics
@pytest.mark.parametrize("red", ["atomic", "two"])
@pytest.mark.parametrize("dt", ["bf16", "f32"])
@pytest.mark.parametrize("C", X.BN_C)
def test_bn_stats(K, monkeypatch, C, dt, red):
    _reduction(monkeypatch, red)
    dtype = DT[dt]
    fams = [f for f in X.X_FAMILIES if not (f == "offset" and dtype == BF16)]
    stride = len(fams) if len(fams) % 2 else len(fams) + 1  # odd: every family meets every option
    seen = set()
    for iM, M in enumerate(X.bn_rows(C)):
        depth = X.bn_plan(M, C)[red]
        for iF, fam in enumerate(fams):
            opt = OPTIONS[(iM * stride + iF) % len(OPTIONS)]
            seen.add(opt)
            exact = fam == "exact"
            seed = 1000 * iM + 10 * iF + C
            x = X.bn_x(fam, M, C, dtype, seed).to(dev)
            res = torch.randn(M, C, generator=X.gen(seed + 1)).to(dtype).to(dev) if opt[1] else None
            dy = X.bn_dy("exact" if exact else "random", M, C, dtype, seed).to(dev)
            pr = _dev(X.bn_params(C, seed, exact=exact))
            _run_case(K, x, x, None, res, dy, pr, opt, depth, exact, red == "two", tag=(M, fam, opt))
    assert len(seen) == len(OPTIONS)
    print("worst error / bound so far:", {k: round(v, 3) for k, v in sorted(WORST.items())})


@pytest.mark.parametrize("red", ["atomic", "two"])
def test_bn_stats_grid_cap(K, monkeypatch, red):
    """C = 512, M = 65,541: want = 16,386 row groups, the grid capped at 2048 (eight rows would need 2049), nine rows
    on the first thread, every one of the BN_PART_MAX partials of a channel written.  bf16; the float64 reference runs
    on the device."""
    _reduction(monkeypatch, red)
    M, C = 65541, 512
    plan = X.bn_plan(M, C)
    if plan == X.bn_plan(M, C, 8, 1024):
        assert plan["grid"] == 2048 and plan["rpt"] == 9
    opt = OPTIONS[0]
    for fam in ("random", "exact"):
        exact = fam == "exact"
        x = X.bn_x(fam, M, C, BF16, 77, lim=7 if exact else 0).to(dev)
        res = torch.randn(M, C, generator=X.gen(78)).bfloat16().to(dev)
        dy = X.bn_dy(fam, M, C, BF16, 79).to(dev)
        pr = _dev(X.bn_params(C, 80, exact=exact))
        _run_case(K, x, x, None, res, dy, pr, opt, plan[red], exact, red == "two", tag=(M, fam))
    print("worst error / bound so far:", {k: round(v, 3) for k, v in sorted(WORST.items())})


# ================================================================================================ splice-on-read
@pytest.mark.parametrize("red", ["atomic", "two"])
@pytest.mark.parametrize("dt", ["bf16", "f32"])
@pytest.mark.parametrize("case", X.SPLICE_CASES, ids=[c[0] for c in X.SPLICE_CASES])
def test_bn_splice(K, monkeypatch, case, dt, red):
    """x' = where(spec, src, x) formed by plain indexing; forward and backward, training and eval: the spliced
    elements of dx exactly +0, everything else within the unspliced bounds evaluated on x'."""
    from iit_amd.ops.splice import PatchSpec
    _reduction(monkeypatch, red)
    name, shape, ranges, layout = case
    dtype = DT[dt]
    N, C, H, W = shape
    M = N * H * W
    st, src4, strides = X.splice_source(shape, layout, dtype, 31)
    spec = PatchSpec(X.spec_dims(shape, ranges, strides))
    hit = X.rows_of(X.splice_mask(shape, ranges)).to(dev)
    assert bool(hit[0].any()) == name.startswith("pivot_in")
    x = X.bn_x("random", M, C, dtype, 33).to(dev)
    xp = torch.where(hit, X.rows_of(src4).to(dev), x)
    st = st.to(dev)
    depth = X.bn_plan(M, C)[red]
    for k, opt in enumerate([OPTIONS[0], OPTIONS[2], OPTIONS[3], OPTIONS[5]]):  # training, eval, training, eval
        res = torch.randn(M, C, generator=X.gen(35 + k)).to(dtype).to(dev) if opt[1] else None
        dy = X.bn_dy("random", M, C, dtype, 37 + k).to(dev)
        pr = _dev(X.bn_params(C, 39 + k))
        _run_case(K, x, xp, hit, res, dy, pr, opt, depth, False, red == "two", splice=(st, spec, H, W),
                  tag=(name, opt))


# ================================================================================================ tile records
@pytest.mark.parametrize("family", ["random", "offset"])
@pytest.mark.parametrize("T,R,C", [(1, 64, 64), (2, 64, 64), (255, 64, 64), (256, 64, 64), (257, 128, 64),
                                   (1000, 64, 64), (8, 128, 8), (8, 128, 2048)])
def test_bn_tiles(K, T, R, C, family):
    """``iit_bn_fwd_tiles`` on records cut from a bf16 activation: T = 1, T < 256, T = 256 and just past it (the
    strided loop plus the tree), T = 1000; ``save``, the running statistics, ``nbt`` and ``y``."""
    M = T * R
    x = X.bn_x(family, M, C, BF16, T + R + C).to(dev)
    cstat = X.tile_records(x, T, R)
    for k, (has_res, relu, mom, nbt0) in enumerate([(True, True, 0.1, 41), (False, False, 1.0, None)]):
        pr = _dev(X.bn_params(C, T + k))
        res = torch.randn(M, C, generator=X.gen(T + 2)).bfloat16().to(dev) if has_res else None
        ref = X.tile_ref(cstat, T, R, pr["rm"], pr["rv"], nbt0, eps=X.BN_EPS, mom=mom)
        X.tile_apply(ref, x, res, pr["w"], pr["b"], relu)
        got = {"y": X.filled((M, C), BF16, dev), "save": X.filled((2 * C,), F32, dev), "rm": pr["rm"].clone(),
               "rv": pr["rv"].clone()}
        nbt = None if nbt0 is None else torch.tensor(nbt0, dtype=torch.long, device=dev)
        K.bn_fwd_tiles(x, res, got["y"], cstat.view(-1), T, R, got["rm"], got["rv"], pr["w"], pr["b"], M, C, X.BN_EPS,
                       relu, got["save"], mom, nbt)
        torch.cuda.synchronize()
        got["nbt"] = None if nbt is None else int(nbt.item())
        bad = _count(X.bn_fwd_check(got, ref))
        assert not bad, (k, bad)
        for key, g in (("mean", got["save"][:C]), ("rstd", got["save"][C:]), ("rm", got["rm"]), ("rv", got["rv"])):
            WORST["tile_" + key] = max(WORST.get("tile_" + key, 0.0), X.worst(g, ref[key], ref["tol_" + key]))
    print("worst error / bound so far:", {k: round(v, 3) for k, v in sorted(WORST.items())})


@pytest.mark.parametrize("family", ["random", "exact"])
def test_conv_epilogue_records(K, family):
    """``K.conv3x3(..., cstat=...)`` at (N, Cin, Cout, hw) = (16, 64, 128, 8) on every tile and split ``conv3x3_ok``
    accepts: ``cstat[0]`` bitwise the first row of each tile of the launch's own bf16 ``y``; ``cstat[1]`` / ``cstat[2]``
    the float64 sums of ``y - p_t`` and its square over the tile's BM rows within ``(BM + 3) E sum |terms|`` -- and bit
    for bit on integer operands whose reference ``sum d^2`` per tile column is below 2^24."""
    N, Cin, Cout, hw = 16, 64, 128, 8
    M = N * hw * hw
    g = X.gen(5)
    CL = torch.channels_last
    if family == "exact":
        x = torch.randint(-1, 2, (N, Cin, hw, hw), generator=g).float()
        w = torch.randint(-1, 2, (Cout, Cin, 3, 3), generator=g).float()
    else:
        x = torch.randn(N, Cin, hw, hw, generator=g)
        w = torch.randn(Cout, Cin, 3, 3, generator=g) / (3 * Cin ** 0.5)
    x = x.bfloat16().to(dev).contiguous(memory_format=CL)
    w = w.bfloat16().to(dev).contiguous(memory_format=CL)
    ran = 0
    for t in range(K.conv3x3_tiles()):
        for sp in (1, 2, 3, 4, 8):
            if not K.conv3x3_ok(N, hw, hw, Cin, Cout, t, sp):
                continue
            ran += 1
            BM = K.conv3x3_rows(t)
            T = M // BM
            y = X.filled((N, Cout, hw, hw), BF16, dev).contiguous(memory_format=CL)
            cstat = X.filled((3 * Cout * T,), F32, dev)
            K.conv3x3(x, w, y, N, hw, hw, Cin, Cout, False, t, sp, cstat=cstat)
            torch.cuda.synchronize()
            rows = y.permute(0, 2, 3, 1).reshape(M, Cout)
            assert not bool(torch.isnan(rows.float()).any()) and not bool((rows == X.filled((1,), BF16, dev)).any())
            rec = cstat.view(3, Cout, T)
            v = rows.double().view(T, BM, Cout)
            p = v[:, 0, :]
            d = v - p[:, None, :]
            s1, s2 = d.sum(1).t(), (d * d).sum(1).t()
            assert not int(X.bad_bits(rec[0].contiguous(), p.t().float().contiguous()).sum()), (t, sp, "pivot")
            if family == "exact":
                assert float(s2.max()) < 2 ** 24 and float(d.abs().sum(1).max()) < 2 ** 24
                assert bool((v == v.round()).all()) and float(v.abs().max()) <= 256
                assert not int(X.bad_bits(rec[1].contiguous(), s1.float().contiguous()).sum()), (t, sp, "S1")
                assert not int(X.bad_bits(rec[2].contiguous(), s2.float().contiguous()).sum()), (t, sp, "S2")
            else:
                tol1 = (BM + 3) * X.E * d.abs().sum(1).t() * X.SLACK
                tol2 = (BM + 3) * X.E * s2 * X.SLACK
                assert not int(X.bad_bound(rec[1], s1, tol1).sum()), (t, sp, "S1")
                assert not int(X.bad_bound(rec[2], s2, tol2).sum()), (t, sp, "S2")
                WORST["cstat_s1"] = max(WORST.get("cstat_s1", 0.0), X.worst(rec[1], s1, tol1))
                WORST["cstat_s2"] = max(WORST.get("cstat_s2", 0.0), X.worst(rec[2], s2, tol2))
    assert ran > 0
    print("tiles x splits run:", ran, {k: round(v, 3) for k, v in sorted(WORST.items()) if k.startswith("cstat")})


# ================================================================================================ refusals
def test_bn_refusals(K, monkeypatch):
    """Each of these returns ``hipErrorInvalidValue`` before any launch (read from the exports: every check precedes
    the first launch), so a RuntimeError is raised and every output keeps its sentinel.  No case would launch with a
    bad pointer."""
    from iit_amd.ops.splice import PatchSpec
    monkeypatch.setattr(K, "CHECK_BOUNDS", False)  # the native refusal, not the Python-side assertion
    M = 16

    def bufs(C, dtype=BF16):
        n = M * C + 8
        return {"x": torch.zeros(n, dtype=dtype, device=dev), "y": X.filled((n,), dtype, dev),
                "save": X.filled((2 * C,), F32, dev), "rm": torch.zeros(C, device=dev), "rv": torch.ones(C, device=dev),
                "w": torch.ones(C, device=dev), "b": torch.zeros(C, device=dev),
                "ws": torch.zeros(K.bn_ws_floats(C), device=dev), "coef": X.filled((2 * C,), F32, dev),
                "dx": X.filled((n,), dtype, dev)}

    def untouched(b):
        torch.cuda.synchronize()
        for k in ("y", "save", "coef", "dx"):
            assert not int(X.bad_bits(b[k], X.filled(tuple(b[k].shape), b[k].dtype, dev)).sum()), k
        assert not bool(b["ws"].view(torch.int32).any())

    def fwd(b, C, x=None, rm="rm", **kw):
        K.bn_fwd(b["x"] if x is None else x, None, b["y"], b["ws"], b[rm] if rm else None, b["rv"], b["w"], b["b"], M,
                 C, 1e-5, True, True, b["save"], 0.1, None, **kw)

    def bwd(b, C, dy=None, **kw):
        K.bn_bwd(b["x"] if dy is None else dy, None, b["x"], torch.zeros(2 * C, device=dev), b["w"], b["ws"], b["coef"],
                 M, C, True, b["dx"], None, None, None, **kw)

    for C in (24, 4):  # 256 % 3 != 0; fewer than 8 channels
        b = bufs(C)
        with pytest.raises(RuntimeError):
            fwd(b, C)
        with pytest.raises(RuntimeError):
            bwd(b, C)
        untouched(b)
    for dtype in (BF16, F32):  # a view offset by one element: not 16-byte aligned
        b = bufs(16, dtype)
        with pytest.raises(RuntimeError):
            fwd(b, 16, x=b["x"][1:])
        with pytest.raises(RuntimeError):
            bwd(b, 16, dy=b["x"][1:])
        untouched(b)
    b = bufs(16)
    with pytest.raises(RuntimeError):
        fwd(b, 16, rm=None)
    untouched(b)
    # a spec whose shape is not (N, C, H, W) of the call: M = 16 rows as (1, 16, 4, 4)
    src = torch.zeros(1, 16, 4, 4, dtype=BF16, device=dev)
    for shape in ((1, 16, 2, 8), (2, 16, 4, 4), (1, 8, 4, 4)):
        spec = PatchSpec(X.spec_dims(shape, [[(0, 1)]] * 4, (0, 16, 4, 1)))
        with pytest.raises(RuntimeError):
            fwd(b, 16, src=src, spec=spec, H=4, W=4)
        with pytest.raises(RuntimeError):
            bwd(b, 16, src=src, spec=spec, H=4, W=4)
    untouched(b)
    cstat = torch.zeros(3 * 16 * 4, device=dev)
    for T, R in ((4, 5), (3, 4), (0, 16)):  # T R != M, T < 1
        with pytest.raises(RuntimeError):
            K.bn_fwd_tiles(b["x"], None, b["y"], cstat, T, R, b["rm"], b["rv"], b["w"], b["b"], M, 16, 1e-5, True,
                           b["save"], 0.1, None)
    untouched(b)

