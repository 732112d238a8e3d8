"""Cases, float64 references, per-element comparators, fp32 restatements and CPU mutants for the perception half's row kernels:
csrc/norm.hip (gr_layernorm, gr_rmsnorm), csrc/pack.hip (gn_stats_kernel + gn_finalize_kernel, fuse_shuffle_kernel in its 16-bit and
e4m3 forms, upsample_coord_kernel) and csrc/ddetr.hip (msda_kernel).  Pure torch: importable without a GPU.  The companion of
tests/attn_cases.py; tests/test_row_cases.py proves every comparator sound and biting on the CPU, tests/test_vision_rows_gpu.py
applies them to the kernels.

Every comparator is PER ELEMENT and has the form
    |got - ref64| <= max(u_kind * |ref64|, floor_kind) + C32[op] * mag
 * u_kind: the unit roundoff of the OUTPUT storage (attn_cases.U; 0 for an fp32 output, kind None).  floor_kind is the storage's
   absolute quantum where it has one: a half below 2^-14 is subnormal (quantum 2^-24), and so is the lo half of a (hi, lo) pair
   below |x| = 2^-3 (groma_amd/ops.py split_pack: |x - (hi + lo)| <= max(2^-22 |x|, 2^-25)); bf16 has fp32's exponent range.
 * mag: a float64 magnitude per element -- the sum of the absolute values of the terms the kernel adds for that element, scaled as
   the kernel scales them (stated at each *_ref64 below).  Where a result depends on a computed COORDINATE (the resamplers, MSDA),
   mag also carries |coordinate| * 2 * (largest |value| next to the sample): bilinear interpolation (zeros padding included) is
   continuous in its coordinates, so an fp32 coordinate that lands on the other side of a pixel boundary than the float64 one moves
   the result by its rounding error times a neighbouring difference, never more.  No element is excluded anywhere.
 * C32[op] = C32_FACTOR x C32_MEASURED[op]: the worst |restatement - ref64| / mag over the op's whole case list, the restatement
   being the kernel's arithmetic in ITS order in fp32 torch without any 16-bit rounding (test_row_cases.py::test_c32_measured
   recomputes every constant and fails when one goes stale); x 4 for what a torch restatement lacks: wave-reduction order where it
   is not restated, fma contraction, the last ulp of the hardware rsqrtf / expf.

The GroupNorm coefficients get a CONDITIONED bound instead (gn_bounds): the statistics kernel's variance is the one-pass
sq / n - mean^2 in fp32, ill-conditioned by design, so a = rstd * gamma is held to C_GN * 2^-24 * (1 + mean^2 / (var + eps))
relative.  That IS the kernel's contract (include/groma_hip.h, gr_gn_finalize), in numbers: with C_GN = 4 x 3.9 the relative error
of a stays below 2^-12 -- a sixteenth of bf16's unit roundoff, the storage the normalised map is written in -- for |mean| / std
<= 16, and below 2^-15 (a sixteenth of fp16's) for |mean| / std <= 5.6; the maps of the region pyramid (conv outputs behind a
GroupNorm-ReLU chain) have |mean| / std of order 1.  At |mean| / std = 128 a is good to 2 digits only (1.5e-2).

The restatements never call torch.sum / matmul in fp32 (their order depends on the CPU's vector width): sums are explicit
sequences of elementwise adds, so the measured constants are the same on every machine.
"""
import math
import zlib
from dataclasses import dataclass

import torch

from tests.attn_cases import F64, U, round_kind

F32 = torch.float32
EPS24 = 2.0 ** -24
KINDS = ("bf16", "fp16", "ref")
UK = dict(U)
UK[None] = 0.0            # fp32 output
FLOOR = {"bf16": 0.0, "fp16": 2.0 ** -25, "ref": 2.0 ** -25, None: 0.0}

C32_FACTOR = 4
# worst |fp32 restatement - ref64| / mag per op over its case list (test_row_cases.py::test_c32_measured)
C32_MEASURED = {"ln": 4.3e-7, "rms": 2.8e-7, "shuffle": 1.2e-7, "upsample": 6.9e-8, "msda": 3.7e-8}
C32 = {k: C32_FACTOR * v for k, v in C32_MEASURED.items()}
# worst relative error of the restated rstd (= of a) in units of 2^-24 * (1 + mean^2 / (var + eps)), over GN_CASES x KINDS
C_GN_MEASURED, C_GN_FACTOR = 3.9, 4
C_GN = C_GN_FACTOR * C_GN_MEASURED


def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def _unravel(flat, shape):
    idx = []
    for n in reversed(shape):
        idx.append(flat % n)
        flat //= n
    return tuple(reversed(idx))


def worst(err, bnd):
    """-> (worst err / bnd, its index).  <= 1 passes.  A non-finite error, or any error where the bound is 0, is inf (1e300-ish)."""
    err, bnd = err.double(), bnd.double().expand_as(err)
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    r = torch.where(err == 0, torch.zeros_like(err), err / bnd.clamp_min(1e-300))
    return float(r.max()), _unravel(int(r.argmax()), tuple(r.shape))


def ubound(ref, kind):
    """the output storage's share of the bound"""
    return (UK[kind] * ref.abs()).clamp_min(FLOOR[kind])


def compare(got, ref, mag, kind, op):
    """the generic comparator -> (worst ratio, index)"""
    return worst((got.double() - ref).abs(), ubound(ref, kind) + C32[op] * mag)


def wave_sum(v):
    """gr_common.h wave_sum on [..., 64]: four DPP rotations inside every 16-lane row, then the rows pairwise.  -> [...]"""
    r = v.reshape(*v.shape[:-1], 4, 16)
    for k in (8, 4, 2, 1):
        r = r + torch.roll(r, k, -1)
    return ((r[..., 0, :] + r[..., 1, :]) + (r[..., 2, :] + r[..., 3, :]))[..., 0]


# ================================================================================================ LayerNorm / RMSNorm
NORM_C_REG = (256, 512, 1024, 2048, 4096)      # norm_rows_kernel<., NV>: every NV instantiation
NORM_C_GEN = (96, 768, 1280, 4352, 100)        # norm_rows_generic_kernel; 100: fp32 output only (C % 32 for the pair build)
NORM_PROFILES = ("zero", "mean50", "const", "spike", "relu")
NORM_CANARY = 1.0e3


@dataclass(frozen=True)
class NormCase:
    name: str
    op: str            # "ln" | "rms"
    rows: int
    C: int
    profile: str
    add: bool = False
    beta: bool = True
    relu: bool = False
    pitched: bool = False
    eps: float = 1e-5

    @property
    def ldx(self):
        return self.C + 8 if self.pitched else self.C

    @property
    def ldo(self):
        return self.C + 32 if self.pitched else self.C

    @property
    def fast(self):     # norm.hip norm_fast_shape
        return self.C % 256 == 0 and self.C <= 4096 and ((self.C >> 8) & ((self.C >> 8) - 1)) == 0

    @property
    def out16(self):
        return self.C % 32 == 0


def _norm_cases():
    out, i = [], 0
    for op in ("ln", "rms"):
        for C in NORM_C_REG + NORM_C_GEN:
            for prof in NORM_PROFILES:
                if op == "rms" and prof == "relu":
                    continue          # gr_rmsnorm has neither add, beta nor relu_in
                ln = op == "ln"
                rows = 37 if prof == "mean50" else (1, 5, 37)[i % 3]     # (one-pass variance errs by one draw of rounding luck per row)
                out.append(NormCase(f"{op}_C{C}_{prof}", op, rows, C, prof, add=ln and bool(i & 1), beta=ln and i % 5 != 0,
                                    relu=prof == "relu", pitched=bool(i & 2)))
                i += 1
    return out


NORM_CASES = _norm_cases()


def make_norm(case):
    """x, add | None [rows, C], gamma, beta | None [C] (fp32 CPU).  Profiles: "zero" std 0.02 (eps = 1e-5 is 2.4 % of the variance: an
    eps in the wrong place shows), "mean50" mean / std = 50, "const" one constant row (x + add constant), "spike" one element per row
    1e4 times the rest, "relu" mostly negative values for relu_in."""
    c, g = case, _gen(case.name)
    z1, z2 = torch.randn((c.rows, c.C), generator=g), torch.randn((c.rows, c.C), generator=g)
    s, m = {"zero": (0.02, 0.0), "mean50": (1.5, 50.0), "const": (2.0, 0.25), "spike": (0.5, 0.0), "relu": (2.0, -0.5)}[c.profile]
    x, a = (s * (m + 0.8 * z1), s * 0.6 * z2) if c.add else (s * (m + z1), None)
    if c.profile == "const":
        x[c.rows // 2] = 0.75
        if a is not None:
            a[c.rows // 2] = 0.5
    if c.profile == "spike":
        for r in range(c.rows):
            col = (7 * r + 3) % c.C
            x[r, col] = 1e4 * s * (1.0 if r % 2 == 0 else -1.0)
            if a is not None:
                a[r, col] = 0.0
    gamma = (0.5 + torch.rand(c.C, generator=g)) * torch.where(torch.rand(c.C, generator=g) < 0.5, -1.0, 1.0)
    beta = torch.randn(c.C, generator=g) if c.beta else None
    return dict(x=x.contiguous(), add=a, gamma=gamma, beta=beta)


def norm_ref64(case, D):
    """-> (out, mag) [rows, C].  LN: out = (v - mean) * rstd * gamma + beta with v = relu?(x + add); the kernel adds v and the mean
    (itself a sum of every v_j / C), both scaled by rstd * gamma, and beta: mag = (|v| + mean_j |v_j|) * rstd * |gamma| + |beta|.
    RMS: out = gamma * v * rstd, one product chain of a well-conditioned sum of squares: mag = |out|."""
    v = D["x"].double()
    if D["add"] is not None:
        v = v + D["add"].double()
    if case.relu:
        v = v.clamp_min(0.0)
    g = D["gamma"].double()
    if case.op == "rms":
        out = g * v / torch.sqrt((v * v).mean(-1, keepdim=True) + case.eps)
        return out, out.abs()
    mean = v.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((v - mean) ** 2).mean(-1, keepdim=True) + case.eps)
    b = D["beta"].double() if D["beta"] is not None else torch.zeros_like(g)
    out = (v - mean) * rstd * g + b
    return out, (v.abs() + v.abs().mean(-1, keepdim=True)) * rstd * g.abs() + b.abs()


def norm_restate(case, D, divisor="C", eps_outside=False, drop_last4=False, one_pass=False, add_ldo=False, relu_after=False,
                 row_off=False):
    """norm_rows_kernel / norm_rows_generic_kernel in fp32 in their order (lane l owns the float4s at l * 4 + 256 i; per-lane
    sequential sums, then wave_sum; mean first, then the variance about the mean).  The keywords are the mutants' handles.
    -> [rows, C] fp32, not rounded to any 16-bit storage."""
    c = case
    R, C = c.rows, c.C
    v = D["x"].clone()
    if D["add"] is not None:
        a = D["add"]
        if add_ldo:      # the add row taken at row * ldo instead of row * ldx, from the pitched buffer the GPU test hands over
            buf = torch.full((R * max(c.ldx, c.ldo) + C,), NORM_CANARY)
            buf[:R * c.ldx].view(R, c.ldx)[:, :C] = a
            a = buf[(torch.arange(R) * c.ldo)[:, None] + torch.arange(C)[None, :]]
        v = v + a
    vo = v.clamp_min(0.0) if c.relu else v                      # what is normalised
    vs = v if (relu_after or not c.relu) else vo                # what the statistics see
    nstat = C - 4 if drop_last4 else C
    P = -(-C // 256) * 256
    div = torch.tensor(float({"C": C, "Cm1": C - 1, "padded": P}[divisor]))
    eps = torch.tensor(c.eps)
    t = torch.zeros((R, P))
    t[:, :nstat] = vs[:, :nstat]
    live = (torch.arange(P) < nstat).view(1, P // 256, 64, 4)
    t = t.view(R, P // 256, 64, 4)
    s = torch.zeros((R, 64))
    sq = torch.zeros((R, 64))
    for i in range(P // 256):
        e = t[:, i]
        s = s + (((e[..., 0] + e[..., 1]) + e[..., 2]) + e[..., 3])
        sq = sq + (((e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]) + e[..., 3] * e[..., 3])
    if c.op == "rms":
        rstd = torch.rsqrt(wave_sum(sq) / div + eps) if not eps_outside else 1.0 / (torch.sqrt(wave_sum(sq) / div) + eps)
        out = D["gamma"] * (vo * rstd[:, None])
    else:
        mean = wave_sum(s) / div
        if one_pass:
            var = (wave_sum(sq) / div - mean * mean).clamp_min(0.0)
        else:
            q = torch.zeros((R, 64))
            for i in range(P // 256):
                for e in range(4):
                    d = (t[:, i, :, e] - mean[:, None]) * live[:, i, :, e]
                    q = q + d * d
            var = wave_sum(q) / div
        rstd = 1.0 / (torch.sqrt(var) + eps) if eps_outside else 1.0 / torch.sqrt(var + eps)
        out = (vo - mean[:, None]) * rstd[:, None] * D["gamma"]
        if D["beta"] is not None:
            out = out + D["beta"]
    return torch.roll(out, 1, 0) if row_off else out


def norm_compare(got, ref, mag, kind, case):
    return compare(got, ref, mag, kind, case.op)


# name -> (restatement keywords, applies(case)).  Judged against the fp32-output comparator (kind None): the GPU test runs every case
# with an fp32 output too, and a divisor off by one in 4096 is a 1.2e-4 effect no 16-bit output can show.
NORM_MUTANTS = {
    "divisor_c_minus_1": (dict(divisor="Cm1"), lambda c: True),
    "divisor_padded_width": (dict(divisor="padded"), lambda c: c.C % 256 != 0),
    "eps_outside_sqrt": (dict(eps_outside=True), lambda c: c.profile == "zero"),     # elsewhere eps is below the fp32 share
    # (the statistics lose the row's last float4; under RMS a spike row's sum of squares is the spike: 4 ordinary elements are 1e-8 of it)
    "generic_last_float4_dropped": (dict(drop_last4=True), lambda c: not c.fast and not (c.op == "rms" and c.profile == "spike")),
    "ln_one_pass_variance": (dict(one_pass=True), lambda c: c.op == "ln" and c.profile == "mean50"),
    "add_read_with_ldo": (dict(add_ldo=True), lambda c: c.add and c.pitched and c.rows > 1),
    "relu_after_statistics": (dict(relu_after=True), lambda c: c.relu),
    "row_written_one_off": (dict(row_off=True), lambda c: c.rows > 1),
}


# ================================================================================================ GroupNorm statistics + finalize
GN_C, GN_IMGS, GN_EPS, GN_ROWS_PER_BLOCK = 128, 2, 1e-5, 512
GN_HW = (33, 512, 520, 1100)
GN_GROUPS = (64, 8, 1)
GN_RATIOS = (0, 4, 32)


@dataclass(frozen=True)
class GnCase:
    name: str
    HW: int
    groups: int
    R: int              # |mean| / std of a group, roughly (gn_ref64 returns the true value)

    @property
    def cpg(self):
        return GN_C // self.groups

    @property
    def nblk(self):
        return -(-self.HW // GN_ROWS_PER_BLOCK)


GN_CASES = [GnCase(f"gn_hw{hw}_g{g}_r{r}", hw, g, r) for hw in GN_HW for g in GN_GROUPS for r in GN_RATIOS]


def make_gn(case, kind, variant=0):
    """x [imgs, HW, C] exact in the storage `kind`, gamma / beta [C].  Channel c of image i has mean s_i * (R + j_ic / 4), j in (-1, 1):
    different per channel inside a group and per image (image 1: the other sign, half the scale).  variant 1: other data in image
    0, the same bits in image 1."""
    g = _gen(case.name)
    z = torch.randn((GN_IMGS, case.HW, GN_C), generator=g)
    j = torch.rand((GN_IMGS, 1, GN_C), generator=g) * 2 - 1
    sc = torch.tensor([1.0, -0.5]).view(2, 1, 1)
    x = sc * (case.R + 0.25 * j + z)
    gamma = (0.5 + torch.rand(GN_C, generator=g)) * torch.where(torch.rand(GN_C, generator=g) < 0.5, -1.0, 1.0)
    beta = torch.randn(GN_C, generator=g)
    if variant:
        x[0] = 1.5 * torch.randn((case.HW, GN_C), generator=g) + 1.0
    return dict(x=round_kind(x, kind), gamma=gamma, beta=beta)


def gn_ref64(case, D):
    """torch.group_norm's statistics in float64: biased variance over HW x cpg elements.  -> dict a, b [imgs, C]; mean, var, mabs
    (mean of |x|) [imgs, C] (a group's value repeated over its channels)"""
    x = D["x"].double().view(GN_IMGS, case.HW, case.groups, case.cpg)
    mean = x.mean((1, 3))
    var = ((x - mean[:, None, :, None]) ** 2).mean((1, 3))
    mabs = x.abs().mean((1, 3))
    mean, var, mabs = (t.repeat_interleave(case.cpg, 1) for t in (mean, var, mabs))
    a = D["gamma"].double() / torch.sqrt(var + GN_EPS)
    return dict(a=a, b=D["beta"].double() - mean * a, mean=mean, var=var, mabs=mabs)


def gn_bounds(ref, D, c_gn=None):
    """-> (bound on a, bound on b) [imgs, C].  rel = C_GN 2^-24 (1 + mean^2 / (var + eps)) is the conditioned bound on rstd, hence on
    a = rstd * gamma.  b = beta - mean * a: the error of a times |mean|, the error of the mean (a sum of n terms of mean magnitude
    mabs, far inside rel * mabs) times |a|, one rounding of the product and one of the difference."""
    rel = (C_GN if c_gn is None else c_gn) * EPS24 * (1.0 + ref["mean"] ** 2 / (ref["var"] + GN_EPS))
    return rel * ref["a"].abs(), rel * ref["mabs"] * ref["a"].abs() + EPS24 * ((ref["mean"] * ref["a"]).abs() + ref["b"].abs())


def gn_partials(case, D, drop_last_block=False):
    """gn_stats_kernel in fp32 in its order: thread (row lane 0..31, 8 channels) adds rows r0 + lane, + 32, ... of its 512-row block in
    sequence; a butterfly over the 8 row lanes of a wave; the 4 waves in sequence.  -> sums [imgs, nblk, C, 2]"""
    nb = case.nblk
    xp = torch.zeros((GN_IMGS, nb * GN_ROWS_PER_BLOCK, GN_C))
    xp[:, :case.HW] = D["x"]
    t = xp.view(GN_IMGS, nb, GN_ROWS_PER_BLOCK // 32, 32, GN_C)
    s = torch.zeros((GN_IMGS, nb, 32, GN_C))
    q = torch.zeros_like(s)
    for it in range(GN_ROWS_PER_BLOCK // 32):
        v = t[:, :, it]
        s, q = s + v, q + v * v
    out = []
    for r in (s, q):
        r = r.view(GN_IMGS, nb, 4, 8, GN_C)
        for _ in range(3):
            r = r[:, :, :, 0::2] + r[:, :, :, 1::2]
        r = r[:, :, :, 0]
        out.append(((r[:, :, 0] + r[:, :, 1]) + r[:, :, 2]) + r[:, :, 3])
    sums = torch.stack(out, -1)
    if drop_last_block:
        sums[:, -1] = 0.0
    return sums


def gn_restate(case, D, drop_last_block=False, n_padded=False, shift_group=False, first64=False, swap_planes=False, ignore_img=False):
    """gn_stats_kernel + gn_finalize_kernel in fp32 in their order (lane l of the finalize wave adds partials e = l, l + 64, ... with
    e = block * cpg + channel-in-group, then wave_sum; var = sq / n - mean^2 clamped at 0).  -> (coef [imgs, 2, C], rstd [imgs, C])"""
    c = case
    sums = gn_partials(c, D, drop_last_block)
    if shift_group:
        sums = torch.roll(sums, -1, 2)
    e = sums.view(GN_IMGS, c.nblk, c.groups, c.cpg, 2).permute(0, 2, 1, 3, 4).reshape(GN_IMGS, c.groups, c.nblk * c.cpg, 2)
    if first64:
        e = e[:, :, :64]
    n_e = e.shape[2]
    pad = -(-n_e // 64) * 64
    ep = torch.zeros((GN_IMGS, c.groups, pad, 2))
    ep[:, :, :n_e] = e
    ep = ep.view(GN_IMGS, c.groups, pad // 64, 64, 2)
    acc = torch.zeros((GN_IMGS, c.groups, 64, 2))
    for i in range(pad // 64):
        acc = acc + ep[:, :, i]
    sm, sq = wave_sum(acc[..., 0]), wave_sum(acc[..., 1])
    n = torch.tensor(float(GN_ROWS_PER_BLOCK * c.nblk if n_padded else c.HW)) * torch.tensor(float(c.cpg))
    mean = sm / n
    var = (sq / n - mean * mean).clamp_min(0.0)
    rstd = 1.0 / torch.sqrt(var + torch.tensor(GN_EPS))
    mean, rstd = mean.repeat_interleave(c.cpg, 1), rstd.repeat_interleave(c.cpg, 1)
    a = rstd * D["gamma"]
    coef = torch.stack((a, D["beta"] - mean * a), 1)
    if swap_planes:
        coef = coef.flip(1)
    if ignore_img:
        coef = coef[:1].expand(GN_IMGS, 2, GN_C).contiguous()
    return coef, rstd


def gn_compare(coef, ref, D):
    """coef [imgs, 2, C] against the conditioned bounds -> (worst ratio, (img, plane, channel))"""
    ba, bb = gn_bounds(ref, D)
    err = torch.stack(((coef[:, 0].double() - ref["a"]).abs(), (coef[:, 1].double() - ref["b"]).abs()), 1)
    return worst(err, torch.stack((ba, bb), 1))


GN_MUTANTS = {
    "last_partial_block_dropped": (dict(drop_last_block=True), lambda c: c.nblk > 1 and c.HW % GN_ROWS_PER_BLOCK != 0),
    "n_is_padded_row_count": (dict(n_padded=True), lambda c: c.HW % GN_ROWS_PER_BLOCK != 0),
    "group_boundary_shifted": (dict(shift_group=True), lambda c: c.groups > 1),
    "only_first_64_partials": (dict(first64=True), lambda c: c.nblk * c.cpg > 64),
    "a_b_planes_swapped": (dict(swap_planes=True), lambda c: True),
    "image_index_ignored": (dict(ignore_img=True), lambda c: True),
}


# ================================================================================================ bilinear align_corners=True
def _resize_ac(src, tapmag, S, dtype, ac_false=False, swap_xy=False):
    """src / tapmag [imgs, Ss, Ss, C] -> ([imgs, S, S, C] resized as fuse_shuffle_kernel / upsample_coord_kernel do it, in `dtype`:
    scale (Ss - 1) / (S - 1), source coordinate scale * y truncated, the upper tap clamped to the last row / column;
    mag [imgs, S, S, C] float64 or None)"""
    Ss = src.shape[1]
    i = torch.arange(S, dtype=dtype)
    if ac_false:
        s = ((i + 0.5) * (Ss / S) - 0.5).clamp_min(0.0)
    else:
        scl = (torch.tensor(float(Ss - 1), dtype=dtype) / torch.tensor(float(S - 1), dtype=dtype)) if S > 1 else torch.tensor(0.0, dtype=dtype)
        s = scl * i
    i0 = s.long().clamp_max(Ss - 1)
    i1 = i0 + (i0 < Ss - 1).long()
    l = s - i0.to(dtype)
    h = 1.0 - l
    sy, sx = s.view(1, S, 1, 1), s.view(1, 1, S, 1)
    ly, lx, hy, hx = l.view(1, S, 1, 1), l.view(1, 1, S, 1), h.view(1, S, 1, 1), h.view(1, 1, S, 1)

    def taps(t):
        if swap_xy:
            t = t.transpose(1, 2)
        r0, r1 = t[:, i0], t[:, i1]
        return r0[:, :, i0], r0[:, :, i1], r1[:, :, i0], r1[:, :, i1]

    v00, v01, v10, v11 = taps(src.to(dtype))
    out = hy * (hx * v00 + lx * v01) + ly * (hx * v10 + lx * v11)
    if tapmag is None:
        return out, None
    m00, m01, m10, m11 = taps(tapmag.double())
    pooled = torch.nn.functional.max_pool2d(tapmag.double().permute(0, 3, 1, 2), 3, 1, 1).permute(0, 2, 3, 1)
    L = torch.maximum(pooled[:, i0][:, :, i0], pooled[:, i1][:, :, i1])
    mag = hy.double() * (hx.double() * m00 + lx.double() * m01) + ly.double() * (hx.double() * m10 + lx.double() * m11)
    return out, mag + 2.0 * (sy.double() + sx.double()) * L


# ================================================================================================ fuse_shuffle (16-bit, e4m3)
SHUF_C, SHUF_IMGS = 64, 2
SHUF_SIZES = ((12, 6, 3), (10, 5, 3))
SHUF_CANARY = 7.0


@dataclass(frozen=True)
class ShufCase:
    name: str
    sizes: tuple
    lvl: int
    coef: tuple          # (tar, top, down): relu(gn(.)) of that source (coef present), or the raw map (null)
    pad: int = 1
    shuffle: int = 1

    @property
    def S(self):
        return self.sizes[self.lvl]

    @property
    def top(self):       # the coarser neighbour, itself at the coarsest level
        return min(self.lvl + 1, 2)

    @property
    def down(self):
        return max(self.lvl - 1, 0)


def _shuf_cases():
    pats = ((1, 1, 1), (0, 0, 0), (1, 0, 1), (0, 1, 0), (1, 1, 0), (0, 0, 1))
    out, i = [], 0
    for sizes in SHUF_SIZES:
        for lvl in range(3):
            for k in range(2):
                p = pats[i % len(pats)]
                out.append(ShufCase(f"shuf_{sizes[0]}_{sizes[1]}_{sizes[2]}_l{lvl}_c{p[0]}{p[1]}{p[2]}_p{1 - k}", sizes, lvl, p, pad=1 - k))
                i += 1
        out.append(ShufCase(f"plain_{sizes[0]}_l{0 if sizes[0] == 12 else 2}_c{int(sizes[0] == 12)}", sizes, 0 if sizes[0] == 12 else 2,
                            (int(sizes[0] == 12), 0, 0), pad=int(sizes[0] != 12), shuffle=0))
    return out


SHUF_CASES = _shuf_cases()
SHUF_Q_INV = 160.0     # e4m3: |value| * q_inv passes 448 for |value| > 2.8, in both directions wherever a raw map is a source


def make_shuf(case, kind):
    """maps [imgs, S_l, S_l, C] of the three levels, exact in `kind`; coef [imgs, 2, C] fp32 per level (a, b different per image)"""
    g = _gen("shuf/" + "_".join(map(str, case.sizes)))       # one pyramid per size triple: every target level sees the same maps
    maps = [round_kind(1.5 * torch.randn((SHUF_IMGS, s, s, SHUF_C), generator=g), kind) for s in case.sizes]
    coef = []
    for _ in case.sizes:
        a = (0.5 + torch.rand((SHUF_IMGS, SHUF_C), generator=g)) * torch.where(torch.rand((SHUF_IMGS, SHUF_C), generator=g) < 0.5, -1.0, 1.0)
        coef.append(torch.stack((a, 0.5 * torch.randn((SHUF_IMGS, SHUF_C), generator=g)), 1).contiguous())
    return dict(maps=maps, coef=coef)


def shuf_eval(case, D, dtype, want_mag=False, swap_src=False, flip_off=False, ac_false=False, swap_xy=False, relu_after=False,
              shift_border=False, other_img_coef=False):
    """fuse_shuffle_kernel's map for the case in `dtype` (float64: the reference; fp32: the restatement, same order as the kernel) ->
    (interior [imgs, S, S, C], mag | None).  A tap's magnitude is |x| |a| + |b| under a coef (x a + b cancels), |x| raw."""
    c, C = case, SHUF_C
    S = c.S

    def source(lvl, use_coef, ch, late_relu):
        x = D["maps"][lvl][..., ch].to(dtype)
        if not use_coef:
            return x, x.abs().double(), False
        cf = D["coef"][lvl].flip(0) if other_img_coef else D["coef"][lvl]
        a, b = cf[:, 0, ch].to(dtype).view(SHUF_IMGS, 1, 1, -1), cf[:, 1, ch].to(dtype).view(SHUF_IMGS, 1, 1, -1)
        y = x * a + b
        return (y if late_relu else y.clamp_min(0.0)), (x.abs() * a.abs() + b.abs()).double(), late_relu

    def block(lvl, use_coef, ch):
        Ss = c.sizes[lvl]
        late = relu_after and Ss != S
        v, tm, pending = source(lvl, use_coef, ch, late)
        if Ss == S:
            return v, tm
        o, m = _resize_ac(v, tm if want_mag else None, S, dtype, ac_false=ac_false, swap_xy=swap_xy)
        return (o.clamp_min(0.0) if pending else o), m

    if not c.shuffle:
        out, mag = block(c.lvl, c.coef[0], torch.arange(C))
    else:
        top, down = (c.top, c.coef[1]), (c.down, c.coef[2])
        if swap_src:
            top, down = down, top
        sgn = -1 if flip_off else 1
        parts = [block(c.lvl, c.coef[0], torch.arange(C // 2)),
                 block(top[0], top[1], (torch.arange(C // 2, 3 * C // 4) + sgn * C // 4) % C),
                 block(down[0], down[1], (torch.arange(3 * C // 4, C) - sgn * C // 4) % C)]
        out = torch.cat([p[0] for p in parts], -1)
        mag = torch.cat([p[1] for p in parts], -1) if want_mag else None
    if shift_border:    # written one pixel off in x and y: the interior's first row and column keep the canary
        o2 = torch.full_like(out, SHUF_CANARY)
        o2[:, 1:, 1:] = out[:, :-1, :-1]
        out = o2
    return out, mag


def shuf_applies(name, c):
    resized = [l for l, _ in ((c.top, 1), (c.down, 2)) if c.sizes[l] != c.S] if c.shuffle else []
    return {
        "top_down_swapped": bool(c.shuffle),
        "source_offset_sign_flipped": bool(c.shuffle),
        "align_corners_false_scale": bool(resized),
        "resize_x_y_swapped": bool(resized),
        # (an integer scale, 5 -> 3, samples pixels: nothing is interpolated and the order of ReLU and resize cannot matter)
        "relu_after_interpolation": bool(c.shuffle) and any(cf and c.sizes[l] != c.S and (c.sizes[l] - 1) % (c.S - 1) != 0
                                                            for l, cf in ((c.top, c.coef[1]), (c.down, c.coef[2]))),
        "border_offset_by_one": True,
        "other_image_coefficients": bool(c.coef[0]) or (bool(c.shuffle) and (bool(c.coef[1]) or bool(c.coef[2]))),
    }[name]


SHUF_MUTANTS = {
    "top_down_swapped": dict(swap_src=True),
    "source_offset_sign_flipped": dict(flip_off=True),
    "align_corners_false_scale": dict(ac_false=True),
    "resize_x_y_swapped": dict(swap_xy=True),
    "relu_after_interpolation": dict(relu_after=True),
    "border_offset_by_one": dict(shift_border=True),
    "other_image_coefficients": dict(other_img_coef=True),
}


# ---- OCP e4m3: the value table (sign 1, exponent 4 bias 7, mantissa 3; 0x7f / 0xff are NaN, no infinities), largest finite 448
def _e4m3_table():
    t = []
    for b in range(256):
        e, m = (b >> 3) & 15, b & 7
        v = float("nan") if (e == 15 and m == 7) else (m / 8.0 * 2.0 ** -6 if e == 0 else (1.0 + m / 8.0) * 2.0 ** (e - 7))
        t.append(-v if b & 0x80 else v)
    return torch.tensor(t, dtype=F64)


E4M3 = _e4m3_table()                                               # byte -> value
E4M3_GRID = torch.unique(E4M3[torch.isfinite(E4M3)])               # the finite values, ascending (-0 and +0 merged)


def e4m3_floor(x):
    return E4M3_GRID[(torch.searchsorted(E4M3_GRID, x.contiguous(), right=True) - 1).clamp(0, len(E4M3_GRID) - 1)]


def e4m3_ceil(x):
    return E4M3_GRID[torch.searchsorted(E4M3_GRID, x.contiguous()).clamp(0, len(E4M3_GRID) - 1)]


def e4m3_round(x):
    """round-to-nearest-even onto the grid (what v_cvt_pk_fp8_f32 does to a value already clamped to +-448); x float64"""
    lo, hi = e4m3_floor(x), e4m3_ceil(x)
    dl, dh = x - lo, hi - x
    even_lo = torch.remainder(torch.round(lo / _e4m3_quantum(lo)), 2) == 0     # the mantissa's last bit
    return torch.where((dl < dh) | ((dl == dh) & even_lo), lo, hi)


def _e4m3_quantum(v):
    a = v.abs().clamp_min(2.0 ** -6)
    return 2.0 ** (torch.floor(torch.log2(a)) - 3)


def shuf_compare_q8(got, ref, mag, q_inv):
    """got: the decoded bytes (E4M3[bytes]) [imgs, S, S, C].  The byte must be one of the two e4m3 values bracketing t = ref * q_inv
    after widening t by the fp32 bound e = C32 mag q_inv + 2^-24 |t| (the product's own rounding) and clamping to +-448: so exactly
    +-448 beyond the clamp.  With [A, B] = [floor(t - e), ceil(t + e)] the ratio is |got - mid| / halfwidth: <= 1 iff got is in [A, B]
    (got is on the grid); where A == B any other value is inf.  -> (worst ratio, index)"""
    t = ref * q_inv
    e = C32["shuffle"] * mag * q_inv + EPS24 * t.abs()
    A, B = e4m3_floor((t - e).clamp(-448.0, 448.0)), e4m3_ceil((t + e).clamp(-448.0, 448.0))
    mid, half = 0.5 * (A + B), 0.5 * (B - A)
    return worst((got.double() - mid).abs(), half)


# ================================================================================================ upsample_coord_pack
UP_C, UP_B, UP_CPAD = 32, 2, 64
UP_CASES_GH = ((6, 6), (6, 12), (6, 24), (5, 7), (4, 9), (3, 1))


@dataclass(frozen=True)
class UpCase:
    name: str
    G: int
    Ho: int


UP_CASES = [UpCase(f"up_g{g}_ho{h}", g, h) for g, h in UP_CASES_GH]


def make_up(case):
    """h fp32 [B, 1 + G*G, C] plus ONE guard row behind the last image ([B*(1+G*G) + 1, C] flat in "flat"): the CLS rows and the guard row
    hold NaN -- a tap that reaches one shows whatever its weight, 0 included (a missing clamp reads them with weight exactly 0)."""
    g = _gen(case.name)
    T = 1 + case.G * case.G
    h = torch.randn((UP_B, T, UP_C), generator=g)
    h[:, 0] = float("nan")
    flat = torch.cat([h.reshape(UP_B * T, UP_C), torch.full((1, UP_C), float("nan"))])
    return dict(h=h, flat=flat)


def linspace_two_sided(n, one_sided=False):
    """upsample_coord_kernel's statement of torch.linspace(-1, 1, n): step = 2 / (n - 1) in fp32, then start + i * step below n // 2 and
    end - (n - 1 - i) * step from there on, each ONE contracted multiply-add (evaluated here exactly in float64 and rounded once to
    fp32, which is what an fma returns); n == 1 gives the start.  torch.linspace on the CPU gives the same bits
    (tests/test_row_cases.py::test_linspace_restatement).  one_sided: start + i * step throughout (the mutant)."""
    if n == 1:
        return torch.tensor([-1.0])
    i = torch.arange(n, dtype=F64)
    step = (torch.tensor(2.0) / torch.tensor(float(n - 1))).double()
    lo, hi = -1.0 + step * i, 1.0 - step * (n - 1 - i)
    return (lo if one_sided else torch.where(i < n // 2, lo, hi)).float()


def up_eval(case, D, dtype, want_mag=False, no_cls_skip=False, no_clamp=False, swap_coord=False, one_sided=False):
    """-> (out [B, Ho, Ho, Cpad] in `dtype`: channels [0, C) the resized map, C the x coordinate, C + 1 the y coordinate, the rest 0;
    mag [B, Ho, Ho, C] | None)"""
    c = case
    G, Ho, T = c.G, c.Ho, 1 + c.G * c.G
    flat = D["flat"]
    if no_clamp:      # per image: its G rows and whatever follows them in memory (the next image's CLS row, the guard row)
        rows = torch.stack([flat[b * T + 1:b * T + 1 + G * G + 1] for b in range(UP_B)])            # [B, G*G + 1, C]
        rows = torch.cat([rows, rows[:, -1:].expand(UP_B, G - 1, UP_C)], 1)                         # pad to (G + 1) * G rows
        src, mag = rows.view(UP_B, G + 1, G, UP_C), None
        i = torch.arange(Ho, dtype=dtype)
        scl = (torch.tensor(float(G - 1), dtype=dtype) / torch.tensor(float(Ho - 1), dtype=dtype)) if Ho > 1 else torch.tensor(0.0, dtype=dtype)
        s = scl * i
        i0 = s.long().clamp_max(G - 1)
        i1c = i0 + (i0 < G - 1).long()
        l = (s - i0.to(dtype))
        ly, lx, hy, hx = l.view(1, Ho, 1, 1), l.view(1, 1, Ho, 1), (1 - l).view(1, Ho, 1, 1), (1 - l).view(1, 1, Ho, 1)
        sd = src.to(dtype)
        r0, r1 = sd[:, i0], sd[:, i0 + 1]
        o = hy * (hx * r0[:, :, i0] + lx * r0[:, :, i1c]) + ly * (hx * r1[:, :, i0] + lx * r1[:, :, i1c])
    else:
        first = 0 if no_cls_skip else 1
        src = torch.stack([flat[b * T + first:b * T + first + G * G] for b in range(UP_B)]).view(UP_B, G, G, UP_C)
        o, mag = _resize_ac(src, src.abs() if want_mag else None, Ho, dtype)
    lin = linspace_two_sided(Ho, one_sided)
    out = torch.zeros((UP_B, Ho, Ho, UP_CPAD), dtype=dtype)
    out[..., :UP_C] = o
    cx, cy = lin.view(1, 1, Ho).to(dtype), lin.view(1, Ho, 1).to(dtype)
    out[..., UP_C], out[..., UP_C + 1] = (cy, cx) if swap_coord else (cx, cy)
    return out, mag


def up_compare(got, ref, mag, kind, case):
    """got [B, Ho, Ho, Cpad].  Features: the generic bound.  Coordinate channels: bit-exact against torch.linspace(-1, 1, Ho) rounded to
    the storage, channel C along x and C + 1 along y; padding channels exactly 0.  -> (worst ratio, index): any coordinate / padding
    mismatch is inf."""
    lin = round_kind(torch.linspace(-1, 1, case.Ho), kind).double()
    exact = torch.zeros_like(ref[..., UP_C:])
    exact[..., 0], exact[..., 1] = lin.view(1, 1, -1), lin.view(1, -1, 1)
    err = (got.double() - torch.cat((ref[..., :UP_C], exact), -1)).abs()
    bnd = torch.cat((ubound(ref[..., :UP_C], kind) + C32["upsample"] * mag, torch.zeros_like(exact)), -1)
    return worst(err, bnd)


# name -> (keywords, applies(case), the storages it is judged in)
UP_MUTANTS = {
    "cls_skip_missing": (dict(no_cls_skip=True), lambda c: True, ("bf16", "ref")),
    "last_row_clamp_missing": (dict(no_clamp=True), lambda c: c.Ho > 1, ("bf16", "ref")),
    "coordinate_channels_swapped": (dict(swap_coord=True), lambda c: c.Ho > 1, ("bf16", "ref")),
    # start + i * step differs from the two-sided form by ONE fp32 rounding in the upper half: judged in the pair storage, the only
    # one that keeps it (bf16 keeps it at Ho = 7 alone: the mid-point is -3e-8 instead of 0); at Ho = 9 step = 0.25 is exact and
    # the two forms agree bit for bit
    "one_sided_linspace": (dict(one_sided=True), lambda c: c.Ho in (6, 12, 24, 7), ("ref",)),
}


# ================================================================================================ MSDA
MSDA_B, MSDA_Q, MSDA_P, MSDA_D = 2, 37, 4, 32
MSDA_SLACK = 8
MSDA_CANARY = 1.0e3
MSDA_CLASSES = ("interior", "band_top", "band_bottom", "band_left", "band_right", "corner_tl", "corner_tr", "corner_bl", "corner_br",
                "outside_top", "outside_bottom", "outside_left", "outside_right")


@dataclass(frozen=True)
class MsdaCase:
    name: str
    heads: int
    Hs: int
    Ws: int
    rdim: int
    ref_batched: int

    @property
    def n(self):          # the tight row: heads * P * 2 offsets + heads * P logits
        return self.heads * MSDA_P * 3

    @property
    def ld(self):
        return self.n + MSDA_SLACK


MSDA_CASES = [MsdaCase(f"msda_h{h}_{hs}x{ws}_r{rd}_b{rb}", h, hs, ws, rd, rb)
              for h in (8, 3) for hs, ws in ((5, 9), (9, 5)) for rd in (2, 4) for rb in (1, 0)]


def _axis_class(t, n):
    """0 outside below (t <= -1), 1 the one-tap band (-1, 0), 2 both taps [0, n - 1], 3 the one-tap band (n - 1, n), 4 outside (t >= n)"""
    return (t > -1).long() + (t >= 0).long() + (t > n - 1).long() + (t >= n).long()


def make_msda(case, canary=MSDA_CANARY):
    """value [B, Hs*Ws, heads, 32], offw [B*Q, ld] (offsets, logits, slack = canary), ref [B*Q | Q, rdim], all fp32.  Every sample's
    pixel coordinate is drawn from the 13 position classes first (interior, the four one-tap bands, the four corner bands, outside on each
    side), the offset that lands it there is then solved from the reference point.  Row (b 0, q 3) carries a +40 logit in every head."""
    c, g = case, _gen(case.name)
    B, Q, H, P = MSDA_B, MSDA_Q, c.heads, MSDA_P
    value = torch.randn((B, c.Hs * c.Ws, H, MSDA_D), generator=g)
    nref = B * Q if c.ref_batched else Q
    ref = 0.1 + 0.8 * torch.rand((nref, c.rdim), generator=g, dtype=F64)
    if c.rdim == 4:
        ref[:, 2:] = 0.2 + 0.4 * torch.rand((nref, 2), generator=g, dtype=F64)
    ref = ref.float()
    # per-axis class of every sample: (row class, column class) from a table that holds each of the 13 classes
    table = torch.tensor([(2, 2)] * 4 + [(1, 2), (3, 2), (2, 1), (2, 3), (1, 1), (1, 3), (3, 1), (3, 3), (0, 2), (4, 2), (2, 0), (2, 4)])
    pick = table[torch.randint(0, len(table), (B, Q, H, P), generator=g)]

    def coord(cls, n):
        u = torch.rand(cls.shape, generator=g, dtype=F64)
        lo = torch.tensor([-3.0, -0.9, 0.0, n - 0.9, n + 0.2], dtype=F64)[cls]
        hi = torch.tensor([-1.2, -0.1, n - 1.0, n - 0.1, n + 2.0], dtype=F64)[cls]
        return lo + (hi - lo) * u

    h_im, w_im = coord(pick[..., 0], c.Hs), coord(pick[..., 1], c.Ws)
    r = (ref.double().view(B, Q, 1, 1, c.rdim) if c.ref_batched else ref.double().view(1, Q, 1, 1, c.rdim).expand(B, Q, 1, 1, c.rdim))
    lx, ly = (w_im + 0.5) / c.Ws, (h_im + 0.5) / c.Hs
    if c.rdim == 2:
        ox, oy = (lx - r[..., 0]) * c.Ws, (ly - r[..., 1]) * c.Hs
    else:
        ox, oy = (lx - r[..., 0]) * P / (r[..., 2] * 0.5), (ly - r[..., 1]) * P / (r[..., 3] * 0.5)
    logits = torch.randn((B, Q, H, P), generator=g)
    logits[0, 3, :, 1] += 40.0
    offw = torch.full((B * Q, c.ld), canary)
    offw[:, :H * P * 2] = torch.stack((ox, oy), -1).float().reshape(B * Q, H * P * 2)
    offw[:, H * P * 2:c.n] = logits.reshape(B * Q, H * P)
    return dict(value=value, offw=offw, ref=ref)


def msda_eval(case, D, dtype, want=None, swap_hw=False, no_half=False, clamp_taps=False, softmax_heads=False, ignore_batched=False,
              no_rdim_half=False, tight_ld=False):
    """The mmcv sampling rule (ms_deform_attn: bilinear, zeros padding, align_corners=False: pixel = loc * size - 0.5; a tap outside the
    map contributes 0) with HF's location arithmetic and the soft-max over the P points, stated directly in `dtype` (float64: the
    reference; fp32: the restatement -- msda_kernel's order).  -> out [B*Q, heads*32]; want="mag" -> (out, mag); want="classes" ->
    the set of position classes the case's samples land in."""
    c = case
    B, Q, H, P, Hs, Ws = MSDA_B, MSDA_Q, c.heads, MSDA_P, c.Hs, c.Ws
    rows = D["offw"].reshape(-1)[:B * Q * c.n].view(B * Q, c.n) if tight_ld else D["offw"][:, :c.n]
    off = rows[:, :H * P * 2].reshape(B, Q, H, P, 2).to(dtype)
    lg = rows[:, H * P * 2:].reshape(B, Q, H, P).to(dtype)
    dim = 2 if softmax_heads else 3
    e = torch.exp(lg - lg.amax(dim, keepdim=True))
    den = e.select(dim, 0)
    for k in range(1, e.shape[dim]):
        den = den + e.select(dim, k)
    w = e / den.unsqueeze(dim)
    ref = D["ref"].to(dtype)
    r = ref.view(B, Q, 1, 1, c.rdim) if (c.ref_batched and not ignore_batched) else ref[:Q].view(1, Q, 1, 1, c.rdim).expand(B, Q, 1, 1, c.rdim)
    rx, ry = r[..., 0], r[..., 1]
    if c.rdim == 2:
        lx, ly = rx + off[..., 0] / Ws, ry + off[..., 1] / Hs
    else:
        half = 1.0 if no_rdim_half else 0.5
        lx, ly = rx + off[..., 0] / P * r[..., 2] * half, ry + off[..., 1] / P * r[..., 3] * half
    Wn, Hn = (Hs, Ws) if swap_hw else (Ws, Hs)
    sh = 0.0 if no_half else 0.5
    w_im, h_im = lx * Wn - sh, ly * Hn - sh
    if want == "classes":
        rc, cc = _axis_class(h_im, Hs), _axis_class(w_im, Ws)
        names = {(2, 2): "interior", (1, 2): "band_top", (3, 2): "band_bottom", (2, 1): "band_left", (2, 3): "band_right",
                 (1, 1): "corner_tl", (1, 3): "corner_tr", (3, 1): "corner_bl", (3, 3): "corner_br"}
        out = set()
        for a, b in set(zip(rc.flatten().tolist(), cc.flatten().tolist())):
            if (a, b) in names:
                out.add(names[(a, b)])
            out |= {n for n, hit in (("outside_top", a == 0), ("outside_bottom", a == 4), ("outside_left", b == 0), ("outside_right", b == 4)) if hit}
        return out
    inside = (h_im > -1) & (w_im > -1) & (h_im < Hs) & (w_im < Ws)
    hl, wl = torch.floor(h_im), torch.floor(w_im)
    lh, lw = h_im - hl, w_im - wl
    uh, uw = 1.0 - lh, 1.0 - lw
    hl, wl = hl.long(), wl.long()
    bi = torch.arange(B).view(B, 1, 1, 1).expand(B, Q, H, P)
    hi = torch.arange(H).view(1, 1, H, 1).expand(B, Q, H, P)
    val = D["value"].to(dtype)

    def tap(y, x, src=val):
        ok = inside if clamp_taps else inside & (y >= 0) & (y <= Hs - 1) & (x >= 0) & (x <= Ws - 1)
        v = src[bi, y.clamp(0, Hs - 1) * Ws + x.clamp(0, Ws - 1), hi]             # [B, Q, H, P, 32]
        return v * ok.unsqueeze(-1)

    def sample(src):
        wt = [(uh * uw), (uh * lw), (lh * uw), (lh * lw)]
        tp = [tap(hl, wl, src), tap(hl, wl + 1, src), tap(hl + 1, wl, src), tap(hl + 1, wl + 1, src)]
        s = wt[0].unsqueeze(-1) * tp[0]
        for k in range(1, 4):
            s = s + wt[k].unsqueeze(-1) * tp[k]
        return s

    def over_points(s):
        acc = s[:, :, :, 0] * w[:, :, :, 0].unsqueeze(-1)
        for p in range(1, P):
            acc = acc + s[:, :, :, p] * w[:, :, :, p].unsqueeze(-1)
        return acc.reshape(B * Q, H * MSDA_D)

    out = over_points(sample(val))
    if want != "mag":
        return out
    # mag: the taps' |value| under the same weights, plus |coordinate| * 2 * the largest |value| in the 4 x 4 pixels around the sample
    av = val.abs()
    grid = torch.nn.functional.pad(av.view(B, Hs, Ws, H, MSDA_D).permute(0, 3, 4, 1, 2), (3, 3, 3, 3))
    pooled = torch.nn.functional.max_pool2d(grid.reshape(B, H * MSDA_D, Hs + 6, Ws + 6), 4, 1).view(B, H, MSDA_D, Hs + 3, Ws + 3)
    L = pooled[bi, hi, :, hl.clamp(-2, Hs) + 2, wl.clamp(-2, Ws) + 2]                 # [B, Q, H, P, 32]
    cm = (rx.abs() + (lx - rx).abs()) * Ws + 0.5 + (ry.abs() + (ly - ry).abs()) * Hs + 0.5
    return out, over_points(sample(av) + 2.0 * cm.unsqueeze(-1) * L)


def msda_compare(got, ref, mag):
    return compare(got, ref, mag, None, "msda")


MSDA_MUTANTS = {
    "hs_ws_swapped": (dict(swap_hw=True), lambda c: True),
    "minus_half_missing": (dict(no_half=True), lambda c: True),
    "border_taps_clamped": (dict(clamp_taps=True), lambda c: True),
    "softmax_across_heads": (dict(softmax_heads=True), lambda c: True),
    "ref_batched_ignored": (dict(ignore_batched=True), lambda c: bool(c.ref_batched)),
    "rdim4_half_missing": (dict(no_rdim_half=True), lambda c: c.rdim == 4),
    "ld_assumed_tight": (dict(tight_ld=True), lambda c: True),
}
