"""The perception half's row kernels against float64, PER OUTPUT ELEMENT, on the cases of tests/row_cases.py: gr_layernorm / gr_rmsnorm
(every NV instantiation and the generic path, row pitches, add / beta / relu_in, in place), gn_stats + gn_finalize (the row-block grid,
the clamped last block, the finalize loops, |mean| / std up to 32), fuse_shuffle in its 16-bit and e4m3 forms, upsample_coord_pack and
msda.  The bounds are those tests/test_row_cases.py proves sound (an fp32 restatement of each kernel passes) and biting (each mutant
of the issue's list is rejected with a factor >= 2 wherever it applies).

Every case runs under ops.precision(kind) for bf16, fp16 and the operand-pair build.  Every output is a view into a larger
canary-filled buffer: the rows before and after it and the pitch gaps stay untouched, and two launches over different canaries give
torch.equal results (every element written, and deterministically)."""
import ctypes
import functools

import pytest
import torch

from tests import row_cases as R

pytestmark = pytest.mark.gpu
PAD = 3                       # canary rows on either side of an output
CANARIES = (7.0, -3.0)        # exact in every storage
Q8_CANARIES = (0x00, 0x3B)    # e4m3 bytes: the engine's zeroed border, and another
F32, F64 = torch.float32, torch.float64
GR_EINVAL = 22


def _vp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _cuda(t):
    return None if t is None else t.contiguous().cuda()


class _Report:
    """collects every case's verdict: one run names all the failures, not the first"""

    def __init__(self, what):
        self.what, self.bad, self.worst = what, [], (0.0, "")

    def add(self, name, ratio, idx, extra=""):
        if ratio > self.worst[0]:
            self.worst = (ratio, name)
        if not ratio <= 1.0:
            self.bad.append(f"{name}: {ratio:.4g} x the bound at {idx} {extra}")

    def done(self):
        print(f"{self.what}: worst ratio {self.worst[0]:.3f} ({self.worst[1]})")
        assert not self.bad, f"{self.what}: {len(self.bad)} case(s) beyond the bound:\n" + "\n".join(self.bad)


def _guarded(rows, width, dtype, run, fill=None):
    """run(out) twice over different canaries, out = rows [PAD, PAD + rows) of a canary-filled [rows + 2 PAD, width] buffer; the guard
    rows stay.  -> [(the raw rows after the launch, its canary)] x 2 for _agree"""
    res = []
    for canary in (fill or CANARIES):
        if dtype == torch.float8_e4m3fn:
            buf = torch.full((rows + 2 * PAD, width), canary, dtype=torch.uint8, device="cuda").view(dtype)
        else:
            buf = torch.full((rows + 2 * PAD, width), canary, dtype=dtype, device="cuda")
        run(buf[PAD:PAD + rows])
        torch.cuda.synchronize()
        raw = buf.view(torch.uint8) if dtype == torch.float8_e4m3fn else buf
        assert bool((raw[:PAD] == canary).all()) and bool((raw[PAD + rows:] == canary).all()), "rows outside `out` were written"
        res.append((raw[PAD:PAD + rows].clone(), canary))
    return res


def _agree(res, written):
    """written: bool [rows, width] -- the elements the kernel owns.  They agree between the launches; all others hold the canary."""
    (a, ca), (b, cb) = res
    assert torch.equal(a[written], b[written]), "two launches differ (an element left unwritten, or a race)"
    assert bool((a[~written] == ca).all()) and bool((b[~written] == cb).all()), "a pitch gap / border element was written"
    return a


# ================================================================================================ LayerNorm / RMSNorm
@functools.lru_cache(maxsize=None)
def _norm_ref(name):
    c = {c.name: c for c in R.NORM_CASES}[name]
    D = R.make_norm(c)
    return c, D, R.norm_ref64(c, D)


def _norm_launch(lib, c, x, add, gamma, beta, out, out16, ldx=None, ldo=None):
    ldx, ldo = ldx or c.ldx, ldo or c.ldo
    if c.op == "ln":
        return lib.gr_layernorm(_vp(x), _vp(add), _vp(gamma), _vp(beta), _vp(out), c.rows, c.C, ldx, ldo, c.eps, int(out16), int(c.relu), _stream())
    return lib.gr_rmsnorm(_vp(x), _vp(gamma), _vp(out), c.rows, c.C, ldx, ldo, c.eps, int(out16), _stream())


def _pitched(t, c):
    if t is None:
        return None
    buf = torch.full((c.rows, c.ldx), R.NORM_CANARY, dtype=F32, device="cuda")
    buf[:, :c.C] = t.cuda()
    return buf


@pytest.mark.parametrize("kind", R.KINDS)
def test_norms(dev, kind):
    """fp32 and 16-bit output of every case; x and add share ldx, out has ldo, canaries in both gaps"""
    from groma_amd import _lib, ops
    rep = _Report(f"norms[{kind}]")
    with ops.precision(kind):
        lib = _lib.load()
        for case in R.NORM_CASES:
            c, D, (ref, mag) = _norm_ref(case.name)
            x, add, gamma, beta = _pitched(D["x"], c), _pitched(D["add"], c), _cuda(D["gamma"]), _cuda(D["beta"])
            x0 = x.clone()
            for out16 in ((False, True) if c.out16 else (False,)):
                spw = ops.SP() if out16 else 1

                def run(out):
                    assert _norm_launch(lib, c, x, add, gamma, beta, out, out16) == 0

                res = _guarded(c.rows, c.ldo * spw, ops.H16() if out16 else F32, run)
                written = torch.zeros((c.rows, c.ldo * spw), dtype=torch.bool, device="cuda")
                written[:, :c.C * spw] = True
                a = _agree(res, written)[:, :c.C * spw]
                got = (ops.from_h16(a) if out16 else a).cpu()
                r, idx = R.norm_compare(got, ref, mag, kind if out16 else None, c)
                rep.add(f"{c.name}/{'h16' if out16 else 'f32'}", r, idx, f"got {float(got[idx]):.7g} ref {float(ref[idx]):.7g} mag {float(mag[idx]):.3g}")
            assert torch.equal(x, x0), "the input was written"
    rep.done()


@pytest.mark.parametrize("kind", R.KINDS)
def test_norm_in_place(dev, kind):
    """fp32 in place on the register path equals out of place bit for bit; the generic path re-reads its row and owes GR_EINVAL,
    with the buffer untouched"""
    from groma_amd import _lib, ops
    by = {c.name: c for c in R.NORM_CASES}
    with ops.precision(kind):
        lib = _lib.load()
        for name in ("ln_C256_spike", "ln_C4096_zero", "rms_C512_zero", "rms_C2048_mean50", "ln_C768_mean50", "ln_C100_zero", "rms_C4352_zero"):
            c, D, _ = _norm_ref(name)
            assert c is by[name]
            x, add, gamma, beta = _cuda(D["x"]), _cuda(D["add"]), _cuda(D["gamma"]), _cuda(D["beta"])
            x0 = x.clone()
            rc = _norm_launch(lib, c, x, add, gamma, beta, x, False, ldx=c.C, ldo=c.C)
            torch.cuda.synchronize()
            if not c.fast:
                assert rc == GR_EINVAL and torch.equal(x, x0), name
                continue
            out = torch.full_like(x0, CANARIES[0])
            assert rc == 0 and _norm_launch(lib, c, x0, add, gamma, beta, out, False, ldx=c.C, ldo=c.C) == 0
            torch.cuda.synchronize()
            assert torch.equal(x, out), f"{name}: in place differs from out of place"


# ================================================================================================ GroupNorm statistics
@functools.lru_cache(maxsize=None)
def _gn_ref(name, kind):
    c = {c.name: c for c in R.GN_CASES}[name]
    D = R.make_gn(c, kind)
    return c, D, R.gn_ref64(c, D)


def _gn_run(ops, c, D, canary):
    """-> (coef [imgs, 2, C], sums [imgs, nblk, C, 2]) through ops.gn_coef with caller-owned, canary-filled buffers"""
    x = ops.to_h16(D["x"].reshape(R.GN_IMGS * c.HW, R.GN_C)).cuda()
    sums = torch.full((R.GN_IMGS, c.nblk, R.GN_C, 2), canary, dtype=F32, device="cuda")
    buf = torch.full((R.GN_IMGS + 2 * PAD, 2, R.GN_C), canary, dtype=F32, device="cuda")
    coef = ops.gn_coef(x, R.GN_IMGS, c.HW, R.GN_C, c.groups, D["gamma"].cuda(), D["beta"].cuda(), R.GN_EPS, sums=sums, coef=buf[PAD:PAD + R.GN_IMGS])
    torch.cuda.synchronize()
    assert bool((buf[:PAD] == canary).all()) and bool((buf[PAD + R.GN_IMGS:] == canary).all()), "rows outside `coef` were written"
    return coef.clone(), sums


@pytest.mark.parametrize("kind", R.KINDS)
def test_gn_coef(dev, kind):
    from groma_amd import ops
    rep = _Report(f"gn_coef[{kind}]")
    with ops.precision(kind):
        for case in R.GN_CASES:
            c, D, ref = _gn_ref(case.name, kind)
            assert ops.gn_stats_blocks(c.HW) == c.nblk
            (c1, s1), (c2, s2) = _gn_run(ops, c, D, CANARIES[0]), _gn_run(ops, c, D, CANARIES[1])
            assert torch.equal(s1, s2), f"{c.name}: a partial [imgs, nblk, C, 2] was left unwritten"
            assert torch.equal(c1, c2), f"{c.name}: two calls give different coefficients"
            # the partial sums themselves: a block's fp32 sum of <= 512 terms is 22 additions deep (16 in a thread, 3 across a wave's
            # row lanes, 3 across the waves), so within 22 * 2^-24 of the sum of magnitudes -- of the block, hence of the image
            want = R.gn_partials(c, D).double()
            tol = 64 * R.EPS24 * torch.stack((D["x"].double().abs().sum(1), (D["x"].double() ** 2).sum(1)), -1).unsqueeze(1)
            assert bool(((s1.cpu().double() - want).abs() <= tol).all()), f"{c.name}: a partial sum is wrong"
            r, idx = R.gn_compare(c1.cpu(), ref, D)
            rep.add(c.name, r, idx, f"got {float(c1[idx]):.7g} |mean|/std {float(ref['mean'][idx[0], idx[2]].abs() / ref['var'][idx[0], idx[2]].sqrt()):.3g}")
            c3, _ = _gn_run(ops, c, R.make_gn(c, kind, variant=1), CANARIES[0])
            assert torch.equal(c3[1], c1[1]), f"{c.name}: image 1's coefficients depend on image 0's data"
            assert not torch.equal(c3[0], c1[0])
    rep.done()


# ================================================================================================ fuse_shuffle
@functools.lru_cache(maxsize=None)
def _shuf_ref(name, kind):
    c = {c.name: c for c in R.SHUF_CASES}[name]
    D = R.make_shuf(c, kind)
    return c, D, R.shuf_eval(c, D, F64, want_mag=True)


def _shuf_run(ops, c, D, q_inv=None):
    """-> interior [imgs, S, S, C * SP] raw storage (bytes for e4m3) of the first of two launches; the border keeps the canary"""
    C, S, Sp = R.SHUF_C, c.S, c.S + 2 * c.pad
    spw = 1 if q_inv is not None else ops.SP()
    srcs = []
    for lvl, use in ((c.lvl, c.coef[0]), (c.top, c.coef[1]), (c.down, c.coef[2])):
        srcs.append((ops.to_h16(D["maps"][lvl].reshape(-1, C)).cuda(), D["coef"][lvl].cuda() if use else None, c.sizes[lvl]))
    tar, top, down = srcs if c.shuffle else (srcs[0], None, None)

    def run(out):
        ops.fuse_shuffle(tar, top, down, out, imgs=R.SHUF_IMGS, C=C, shuffle=bool(c.shuffle), pad=c.pad, q_inv=q_inv)

    rows = R.SHUF_IMGS * Sp * Sp
    res = _guarded(rows, C * spw, torch.float8_e4m3fn if q_inv is not None else ops.H16(), run, fill=Q8_CANARIES if q_inv is not None else None)
    written = torch.zeros((R.SHUF_IMGS, Sp, Sp, C * spw), dtype=torch.bool, device="cuda")
    written[:, c.pad:c.pad + S, c.pad:c.pad + S] = True
    a = _agree(res, written.view(rows, C * spw))
    return a.view(R.SHUF_IMGS, Sp, Sp, C * spw)[:, c.pad:c.pad + S, c.pad:c.pad + S]


@pytest.mark.parametrize("kind", R.KINDS)
def test_fuse_shuffle(dev, kind):
    """the 16-bit writer: every level a target, coef present and null per source, pad 1 and 0, shuffle 0; the pre-filled border stays"""
    from groma_amd import ops
    rep = _Report(f"fuse_shuffle[{kind}]")
    with ops.precision(kind):
        for case in R.SHUF_CASES:
            c, D, (ref, mag) = _shuf_ref(case.name, kind)
            got = ops.from_h16(_shuf_run(ops, c, D)).cpu()
            r, idx = R.compare(got, ref, mag, kind, "shuffle")
            rep.add(c.name, r, idx, f"got {float(got[idx]):.7g} ref {float(ref[idx]):.7g} mag {float(mag[idx]):.3g}")
    rep.done()


@pytest.mark.parametrize("kind", R.KINDS)
def test_fuse_shuffle_e4m3(dev, kind):
    """the e4m3 writer (st8q): each byte one of the two e4m3 values bracketing ref * q_inv, exactly +-448 beyond the clamp, the border
    untouched (exactly 0 over the zeroed buffer).  The operand-pair build has no e4m3 path: GR_EINVAL."""
    from groma_amd import ops
    rep = _Report(f"fuse_shuffle_e4m3[{kind}]")
    with ops.precision(kind):
        for case in R.SHUF_CASES:
            c, D, (ref, mag) = _shuf_ref(case.name, kind)
            if kind == "ref":
                with pytest.raises(RuntimeError, match=f"code {GR_EINVAL}"):
                    _shuf_run(ops, c, D, q_inv=R.SHUF_Q_INV)
                continue
            byte = _shuf_run(ops, c, D, q_inv=R.SHUF_Q_INV).cpu()
            got = R.E4M3[byte.long()]
            r, idx = R.shuf_compare_q8(got, ref, mag, R.SHUF_Q_INV)
            rep.add(c.name, r, idx, f"byte {int(byte[idx]):#04x} = {float(got[idx]):g}, ref * q_inv {float(ref[idx]) * R.SHUF_Q_INV:.6g}")
            t = ref * R.SHUF_Q_INV
            assert bool((got[t > 448.0 * 1.001] == 448.0).all()) and bool((got[t < -448.0 * 1.001] == -448.0).all()), c.name
    rep.done()


# ================================================================================================ upsample_coord_pack
@functools.lru_cache(maxsize=None)
def _up_ref(name):
    c = {c.name: c for c in R.UP_CASES}[name]
    D = R.make_up(c)
    return c, D, R.up_eval(c, D, F64, want_mag=True)


@pytest.mark.parametrize("kind", R.KINDS)
def test_upsample_coord_pack(dev, kind):
    """Ho = G, 2G, 4G, odd Ho, Ho = 1; the CLS rows (and a guard row behind the last image) hold NaN; coordinate channels bit-exact"""
    from groma_amd import ops
    rep = _Report(f"upsample_coord_pack[{kind}]")
    with ops.precision(kind):
        for case in R.UP_CASES:
            c, D, (ref, mag) = _up_ref(case.name)
            flat = D["flat"].cuda()
            h = flat[:-1].view(R.UP_B, 1 + c.G * c.G, R.UP_C)
            rows, width = R.UP_B * c.Ho * c.Ho, R.UP_CPAD * ops.SP()
            res = _guarded(rows, width, ops.H16(), lambda out: ops.upsample_coord_pack(h, c.G, c.Ho, R.UP_CPAD, out=out))
            a = _agree(res, torch.ones((rows, width), dtype=torch.bool, device="cuda"))
            got = ops.from_h16(a).cpu().view(R.UP_B, c.Ho, c.Ho, R.UP_CPAD)
            assert torch.equal(torch.linspace(-1, 1, c.Ho, device="cuda").cpu(), torch.linspace(-1, 1, c.Ho)), "torch.linspace: device != host"
            r, idx = R.up_compare(got, ref, mag, kind, c)
            rep.add(c.name, r, idx, f"got {float(got[idx]):.9g}" + (f" ref {float(ref[idx]):.9g}" if idx[3] < R.UP_C else f" linspace {torch.linspace(-1, 1, c.Ho).tolist()}"))
    rep.done()


# ================================================================================================ MSDA
@functools.lru_cache(maxsize=None)
def _msda_ref(name):
    c = {c.name: c for c in R.MSDA_CASES}[name]
    D = R.make_msda(c)
    return c, D, R.msda_eval(c, D, F64, want="mag")


@pytest.mark.parametrize("kind", R.KINDS)
def test_msda(dev, kind):
    """Hs != Ws, rdim 2 and 4, ref_batched 1 and 0, ld with slack (canaries in it), samples in every position class, a +40 logit"""
    from groma_amd import _lib, ops
    rep = _Report(f"msda[{kind}]")
    with ops.precision(kind):
        lib = _lib.load()
        for case in R.MSDA_CASES:
            c, D, (ref, mag) = _msda_ref(case.name)
            value, refp = D["value"].cuda(), D["ref"].cuda()
            offws = []
            for canary in (R.MSDA_CANARY, -77.0):
                o = D["offw"].clone()
                o[:, c.n:] = canary
                offws.append(o.cuda())

            def run(out):
                offw = offws.pop(0)
                assert lib.gr_msda_f32(_vp(value), _vp(offw), _vp(refp), _vp(out), R.MSDA_B, R.MSDA_Q, c.heads, R.MSDA_P, c.Hs, c.Ws,
                                       c.ld, c.rdim, c.ref_batched, _stream()) == 0
                torch.cuda.synchronize()

            rows, width = R.MSDA_B * R.MSDA_Q, c.heads * R.MSDA_D
            a = _agree(_guarded(rows, width, F32, run), torch.ones((rows, width), dtype=torch.bool, device="cuda"))
            got = a.cpu()
            r, idx = R.msda_compare(got, ref, mag)
            rep.add(c.name, r, idx, f"got {float(got[idx]):.7g} ref {float(ref[idx]):.7g} mag {float(mag[idx]):.3g}")
    rep.done()
