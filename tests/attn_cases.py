"""Cases, float64 reference, per-element comparator and CPU mutants for the attention kernels (csrc/attention.hip: attention_kernel
in its slot, paged and operand-pair forms; csrc/decode.hip: decode_attention_kernel).  Pure torch: importable without a GPU.

 * make_case(case, profile, kind) builds q / k / v that are exact in the operand storage `kind` ("bf16" | "fp16" | "ref" = (hi, lo)
   pairs of halves); the reference is always computed from these rounded values.  Everything the kernel must not see -- K rows and V
   columns from the row's last visible key to kv_stride, the sink page, the unused tail of a row's last page, pages in no table --
   holds FINITE sentinels: V = 1e3, K = a row whose score beats every real key of the row.  A masked probability is exactly 0 in the
   kernel, so sentinels cost a correct kernel nothing and a leaking one everything.
 * score profiles: "flat" (randn), "recent" (key j gets +BETA * (j - mid) after scaling: the last visible keys carry the weight and
   every 64-key tile raises the running max, so the online-softmax rescale fires on every tile), "early" (the ramp flipped: key 0
   dominates, alpha stays 1, a wrong OLD tile or page is visible from every later row).  In all three q's channel 0 is the constant
   C_Q (this is what lets one sentinel K row beat the real keys for every query); under RoPE the tables leave the channel pair
   (0, hd/2) unrotated (cos 1, sin 0) and are random elsewhere, so a wrong position cannot cancel.
 * ref64(q, k, v, visible) -> (out, mag): float64 soft-max attention and mag = softmax @ |v|, the comparator's scale.  A row with no
   visible key gives 0 (the contract of gr_attention_bf16 and gr_decode_attention, include/groma_hip.h).
 * compare(): componentwise |got - out| <= (roundings * u + C32) * mag, u the unit roundoff of the storage (derived, not measured).
 * MUTANTS: deliberately wrong visibility masks / references, CPU only (tests/test_attn_cases.py proves the comparator rejects each
   of them on every case it applies to; a "past-the-table tile not going to page 0" mutant is NOT among them: inside the argument
   contract q_pos0 + Lq <= table_ld * 64 the readers never index past the table, so it cannot be observed).
"""
import math
import zlib
from dataclasses import dataclass, field

import torch

F64 = torch.float64
BETA, C_Q = 0.125, 4.0      # ramp slope per key after scaling; q's constant channel 0
V_SENTINEL = 1.0e3          # exact in bf16 and fp16
K_SENTINEL_MARGIN = 30.0    # a sentinel key's scaled score lies this far above the largest ramp bonus

# unit roundoff of the operand storage: bf16 has 8 significand bits, IEEE half 11, a (hi, lo) pair of halves 22
U = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11, "ref": 2.0 ** -22}
# fp32 share of the bound: accumulation order, exp2, and above all the fp32 rounding of scores whose ramp term reaches |score * scale|
# ~ 64 (raw dot products of magnitude ~500 summed in fp32 accumulators, as the MFMA does).  MEASURED, not tuned on the kernel: the worst
# |emulate(roundings=False) - ref64| / mag -- the fp32 tile-wise restatement without any 16-bit rounding -- over every case x profile
# of this module is 3.39e-5 (tests/test_attn_cases.py::test_c32_measured recomputes it and fails if the constant goes stale); x 4 for
# what the torch restatement lacks (MFMA summation order, the last ulp of the hardware exp2).  That is 1.7 % of bf16's 2u and 14 % of
# fp16's: it cannot hide a mutant there (they are rejected against the bf16 bound with a factor of 2 to spare); in the pair build
# (2u = 4.8e-7) it IS the bound.
C32_MEASURED, C32_FACTOR = 3.4e-5, 4
C32 = C32_FACTOR * C32_MEASURED


def round_kind(x, kind):
    """fp32 values -> the nearest values the storage holds, as fp32 (exact)"""
    x = x.float()
    if kind == "bf16":
        return x.bfloat16().float()
    hi = x.clamp(-65504.0, 65504.0).half()
    if kind == "fp16":
        return hi.float()
    lo = (x - hi.float()).half()
    return hi.float() + lo.float()


@dataclass(frozen=True)
class Case:
    name: str
    B: int
    H: int
    Lq: int
    hd: int
    Skv: int                 # host Skv (with pos: the capacity bound max(pos) + Lq)
    kv_stride: int
    causal: bool = True
    q_pos0: int = 0          # host argument (ignored with pos)
    pos: tuple = None        # pos_dev values: B entries (pos_stride 1) or one shared counter (pos_stride 0)
    kv_len: tuple = None
    fused: bool = False      # q read in place from the fused projection rows [B*Lq, q_ld] + RoPE at q_pos0_b + i
    q_ld: int = 0
    paged: bool = False      # also run through gr_attention_paged (Skv_b = q_pos0_b + Lq, causal)
    # mutant name -> reason: the mutant changes this case's mask but no profile can show it
    exempt: dict = field(default_factory=dict, hash=False, compare=False)

    @property
    def pos_stride(self):
        return 0 if self.pos is None or len(self.pos) == 1 else 1

    def pos0(self, b):
        return self.q_pos0 if self.pos is None else self.pos[b * self.pos_stride]

    def skv(self, b):
        return self.Skv if self.pos is None else self.pos0(b) + self.Lq

    def kvmax(self, b):
        return self.skv(b) if self.kv_len is None else max(0, min(self.skv(b), self.kv_len[b]))

    @property
    def decode(self):        # the Lq = 1 cases also run through gr_decode_attention(_paged)
        return self.Lq == 1 and self.causal and not self.fused

    @property
    def table_ld(self):      # one entry more than any row needs: every row's table is shorter than table_ld
        return self.kv_stride // 64 + 1


def _c(name, B, H, Lq, hd, Skv, stride, **kw):
    return Case(name, B, H, Lq, hd, Skv, stride, **kw)


CASES = [
    # ---- non-causal (ViT): Skv on and around the 64-key tile, the DINOv2 length, the LLaMA length
    _c("vit_skv1", 1, 2, 1, 64, 1, 64, causal=False),
    _c("vit_skv63", 1, 2, 63, 64, 63, 64, causal=False),
    _c("vit_skv64", 1, 2, 64, 64, 64, 128, causal=False),
    _c("vit_skv65", 1, 2, 65, 64, 65, 128, causal=False),
    _c("vit_1025", 1, 2, 1025, 64, 1025, 1088, causal=False),
    _c("noncausal_582", 1, 2, 582, 128, 582, 640, causal=False),
    _c("vit_kvlen", 3, 1, 130, 64, 130, 192, causal=False, kv_len=(130, 129, 64)),
    # ---- causal, small Lq: partial 16-row q-tiles, a wave with no rows, a block with one row; q_pos0 around a tile edge
    _c("lq15_bh15", 3, 5, 15, 64, 15, 64),
    _c("lq16_pos1", 1, 2, 16, 128, 17, 64, q_pos0=1, paged=True),
    _c("lq17_pos63", 1, 2, 17, 128, 80, 128, q_pos0=63, paged=True),
    _c("lq32_pos64", 2, 1, 32, 128, 96, 128, q_pos0=64, paged=True),
    _c("lq33_pos65", 1, 2, 33, 64, 98, 192, q_pos0=65, paged=True),
    # ---- Lq = 1 (also through the decode kernels)
    _c("dec_pos320", 2, 2, 1, 128, 321, 384, q_pos0=320, paged=True),
    _c("dec_ragged", 3, 2, 1, 64, 65, 128, pos=(0, 63, 64), paged=True,
       exempt={"no_alpha_rescale": "the only second tile is row 2's single key 64, which does not raise that row's running max: alpha is 1"}),
    _c("dec_kvlen", 4, 1, 1, 128, 201, 256, q_pos0=200, kv_len=(0, 1, 64, 129), paged=True),
    _c("dec_shared_ctr", 2, 3, 1, 128, 130, 192, pos=(129,), kv_len=(130, 65), paged=True),
    # ---- more than one 128-row query block
    _c("lq257_kvlen", 2, 2, 257, 128, 257, 320, kv_len=(257, 256)),
    _c("lq256_pos130", 3, 1, 256, 128, 386, 448, q_pos0=130, kv_len=(320, 321, 319), paged=True),
    _c("lq383_hd64", 1, 2, 383, 64, 383, 448),
    _c("llama_582_pad", 2, 3, 582, 128, 582, 640, kv_len=(545, 582)),
    _c("lq127", 1, 2, 127, 128, 127, 128),
    _c("lq128_hd64", 1, 3, 128, 64, 128, 128),
    # ---- device positions: ragged rows (pos_stride 1), one shared counter (pos_stride 0)
    _c("ragged_lq17", 4, 2, 17, 128, 217, 256, pos=(100, 64, 0, 200), paged=True),
    _c("ragged_lq130", 4, 1, 130, 128, 322, 384, pos=(192, 70, 1, 63), kv_len=(322, 197, 131, 190), paged=True),
    _c("shared_ctr_lq33", 2, 2, 33, 64, 98, 128, pos=(65,), paged=True),
    # ---- kv_len[b] < q_pos0 + 1: every query of the row sees the same keys; a row with no visible key
    _c("kvlen_below_pos", 3, 1, 40, 128, 190, 192, q_pos0=150, kv_len=(128, 65, 0), paged=True),
    # ---- q in place in the fused projection rows + RoPE
    _c("fused_lq70", 2, 2, 70, 128, 70, 128, fused=True, q_ld=3 * 2 * 128),
    _c("fused_pos167", 1, 2, 33, 64, 200, 256, q_pos0=167, fused=True, q_ld=3 * 2 * 64 + 64, paged=True),
    _c("fused_ragged", 3, 4, 17, 64, 145, 192, pos=(3, 128, 77), fused=True, q_ld=3 * 4 * 64, paged=True),
    _c("fused_lq150_pad", 2, 4, 150, 128, 150, 192, kv_len=(150, 141), fused=True, q_ld=3 * 4 * 128),
]
PROFILES = ("flat", "recent", "early")
KINDS = ("bf16", "fp16", "ref")


def check_contract(case):
    """the argument contract of gr_attention_bf16 / gr_attention_paged / gr_decode_attention (nothing here may fault a GPU)"""
    c = case
    assert c.hd in (64, 128) and c.B > 0 and c.H > 0 and c.Lq > 0 and c.Skv > 0
    assert c.kv_stride % 64 == 0 and c.kv_stride >= c.Skv
    assert all(c.pos0(b) >= 0 and c.skv(b) <= c.kv_stride for b in range(c.B))
    if c.pos is not None:
        assert len(c.pos) in (1, c.B) and c.Skv == max(c.pos) + c.Lq
    if c.kv_len is not None:
        assert len(c.kv_len) == c.B and min(c.kv_len) >= 0
    if c.fused:
        assert c.q_ld % 32 == 0 and c.q_ld >= 3 * c.H * c.hd      # (% 32: the operand-pair build)
    if c.paged:
        assert c.causal and c.table_ld * 64 <= 8192
        assert all(c.skv(b) == c.pos0(b) + c.Lq and c.pos0(b) + c.Lq <= c.table_ld * 64 for b in range(c.B))
    if c.decode:
        assert c.Skv <= 8192 and all(c.pos0(b) + 1 <= c.Skv for b in range(c.B))


# ------------------------------------------------------------------------------------------------ visibility
def limits(case, causal_off=0, kvlen_off=0, skv_off=0, row_shift=0, swap_kvlen=False, swap_pos=False):
    """[B, Lq] int64: keys [0, limit) are visible to query i of row b -- attention_kernel's `limit[u]`.  The keyword arguments are
    the mutants' handles (all 0 / False: the contract)."""
    i = torch.arange(case.Lq)
    out = []
    for b in range(case.B):
        partner = b ^ 1 if (b ^ 1) < case.B else b
        bp, bk = (partner if swap_pos else b), (partner if swap_kvlen else b)
        p0 = case.pos0(bp)
        kvmax = (p0 + case.Lq if case.pos is not None else case.Skv) + skv_off
        if case.kv_len is not None:
            kvmax = min(kvmax, case.kv_len[bk] + kvlen_off)
        lim = torch.full((case.Lq,), kvmax)
        if case.causal:
            lim = torch.minimum(lim, p0 + (i + row_shift).clamp(0, case.Lq - 1) + 1 + causal_off)
        out.append(lim.clamp(0, case.kv_stride))
    return torch.stack(out)


def visible(limit, S):
    """[B, 1, Lq, S] bool from limits()"""
    return (torch.arange(S, device=limit.device)[None, None, :] < limit[:, :, None]).unsqueeze(1)


# ------------------------------------------------------------------------------------------------ inputs
def rope(x, cos, sin, pos):
    """HF rotate_half on x [B, H, Lq, hd] at positions pos [B, Lq]; tables [npos, hd/2]; in x's dtype"""
    half = x.shape[-1] // 2
    c = torch.cat([cos[pos], cos[pos]], -1).to(x.dtype).unsqueeze(1)
    s = torch.cat([sin[pos], sin[pos]], -1).to(x.dtype).unsqueeze(1)
    return x * c + torch.cat([-x[..., half:], x[..., :half]], -1) * s


def positions(case, use_pos0=True):
    i = torch.arange(case.Lq)
    return torch.stack([i + (case.pos0(b) if use_pos0 else 0) for b in range(case.B)])


def make_case(case, profile, kind):
    """dict of CPU tensors: q [B,H,Lq,hd] (before RoPE), k / v [B,H,kv_stride,hd] (fp32 holding values exact in `kind`), cos / sin and
    qbuf [B*Lq, q_ld] when fused, q_eff (float64: what the scores are taken with -- q, or the rotated q as the kernel holds it)."""
    c = case
    g = torch.Generator().manual_seed(zlib.crc32(f"{c.name}/{profile}".encode()))
    scale = c.hd ** -0.5
    q = torch.randn((c.B, c.H, c.Lq, c.hd), generator=g)
    k = torch.randn((c.B, c.H, c.kv_stride, c.hd), generator=g)
    v = torch.randn((c.B, c.H, c.kv_stride, c.hd), generator=g)
    q[..., 0] = C_Q
    kmax_all = max(c.kvmax(b) for b in range(c.B))
    bonus_max = 0.0
    if profile != "flat":
        j = torch.arange(c.kv_stride, dtype=torch.float32)
        bonus = BETA * (j - kmax_all // 2) * (1.0 if profile == "recent" else -1.0)
        k[..., 0] = bonus / (C_Q * scale)
        bonus_max = BETA * (kmax_all - kmax_all // 2)
    if c.paged and c.B >= 2:   # row 1 holds row 0's keys on the leading whole pages both can see: the paged form shares those pages
        n = 64 * (min(c.kvmax(0), c.kvmax(1)) // 64)
        k[1, :, :n], v[1, :, :n] = k[0, :, :n], v[0, :, :n]
    k_sentinel = (bonus_max + K_SENTINEL_MARGIN) / (C_Q * scale)
    for b in range(c.B):
        m = c.kvmax(b)
        k[b, :, m:] = 0.0
        k[b, :, m:, 0] = k_sentinel
        v[b, :, m:] = V_SENTINEL
    D = dict(k_sentinel=k_sentinel, q=round_kind(q, kind), k=round_kind(k, kind), v=round_kind(v, kind), scale=scale, kind=kind, profile=profile)
    assert float((D["q"][..., 0] - C_Q).abs().max()) == 0.0
    D["q_eff"] = D["q"].double()
    if c.fused:
        npos = c.kv_stride
        cos, sin = torch.randn((npos, c.hd // 2), generator=g), torch.randn((npos, c.hd // 2), generator=g)
        cos[:, 0], sin[:, 0] = 1.0, 0.0     # the pair (0, hd/2) stays put: channel 0 keeps the profile's constant
        qbuf = round_kind(torch.randn((c.B * c.Lq, c.q_ld), generator=g), kind)
        qbuf[:, : c.H * c.hd] = D["q"].permute(0, 2, 1, 3).reshape(c.B * c.Lq, c.H * c.hd)
        D.update(cos=cos.contiguous(), sin=sin.contiguous(), qbuf=qbuf.contiguous())
        D["q_eff"] = rotated_q(D, c, F64)
    return D


def rotated_q(D, case, dtype, use_pos0=True):
    """the rotated q as the kernel holds it: rotated in `dtype` (the kernel: fp32), then rounded to the 16-bit storage (the pair
    build keeps ~22 bits: not rounded here)"""
    r = rope(D["q"].to(dtype), D["cos"], D["sin"], positions(case, use_pos0))
    return (round_kind(r, D["kind"]) if D["kind"] != "ref" else r).double()


def build_pages(D, case, seed=0):
    """slot caches -> (k_pool [P+1+2,H,64,hd], vt_pool [P+1+2,H,hd,64], table int32 [B, table_ld]) over a random page permutation.
    Page 0 (the sink) and two pages in no table hold sentinels; row 1 maps the pages it shares with row 0 (make_case made the keys
    equal there); every row's table ends in sink entries."""
    c = case
    g = torch.Generator().manual_seed(1000 + seed + c.Lq)
    need = [-(-(c.pos0(b) + c.Lq) // 64) for b in range(c.B)]
    share = 0
    if c.B >= 2:
        share = min(c.kvmax(0), c.kvmax(1)) // 64
    P = sum(need) - share
    perm = (torch.randperm(P + 2, generator=g) + 1).tolist()
    kp = torch.zeros((P + 3, c.H, 64, c.hd))
    kp[..., 0] = D["k_sentinel"]
    kp = round_kind(kp, D["kind"])
    vp = torch.full((P + 3, c.H, c.hd, 64), V_SENTINEL)
    table = torch.zeros((c.B, c.table_ld), dtype=torch.int32)
    for b in range(c.B):
        for t in range(need[b]):
            if b == 1 and t < share:
                table[1, t] = table[0, t]
                continue
            pg = perm.pop()
            table[b, t] = pg
            kp[pg] = D["k"][b, :, 64 * t:64 * t + 64]
            vp[pg] = D["v"][b, :, 64 * t:64 * t + 64].transpose(1, 2)
    return kp, vp, table


def gather_pages(kp, vp, table, case, page_of=None):
    """what a reader sees through the table: k / v [B,H,kv_stride,hd].  page_of(b, t) -> table coordinates (b', t') is the paged
    mutants' handle; a tile past the table reads the sink page."""
    ld = table.shape[1]
    ks, vs = [], []
    for b in range(case.B):
        kb, vb = [], []
        for t in range(case.kv_stride // 64):
            bb, tt = page_of(b, t) if page_of else (b, t)
            pg = int(table[bb, tt]) if 0 <= tt < ld else 0
            kb.append(kp[pg])
            vb.append(vp[pg].transpose(1, 2))
        ks.append(torch.cat(kb, 1))
        vs.append(torch.cat(vb, 1))
    return torch.stack(ks), torch.stack(vs)


# ------------------------------------------------------------------------------------------------ reference, comparator
def ref64(q, k, v, vis, scale=None):
    """float64: out = softmax(masked q.k^T * scale) @ v and mag = softmax(...) @ |v|, both [B,H,Lq,hd]; vis bool [B,1|H,Lq,S];
    a row with no visible key gives 0"""
    q, k, v = q.double(), k.double(), v.double()
    scale = q.shape[-1] ** -0.5 if scale is None else scale
    s = (q @ k.transpose(-1, -2)) * scale
    s = s.masked_fill(~vis, float("-inf"))
    m = s.amax(-1, keepdim=True)
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    p = torch.exp(s - m)
    l = p.sum(-1, keepdim=True)
    p = p / torch.where(l > 0, l, torch.ones_like(l))
    return p @ v, p @ v.abs()


def bound_factor(kind, roundings=2):
    """roundings: 2 for attention_kernel (P is rounded to the storage before the P.V MFMA -- the row sum is taken from the unrounded
    fp32 values, so normalising adds nothing -- and the output is rounded once); 1 for decode_attention_kernel (P stays fp32)"""
    return roundings * U[kind] + C32


def compare(got, out, mag, kind, roundings=2):
    """-> (worst ratio |got - out| / bound, its (b, h, i, d)); bound = (roundings * u + C32) * mag PER ELEMENT.  ratio <= 1 passes; a
    non-finite result, or any error where the bound is 0 (a row with no visible key), is inf."""
    err = (got.double() - out).abs()
    bnd = bound_factor(kind, roundings) * mag
    ratio = torch.where(err <= bnd, err / bnd.clamp_min(1e-300), torch.where(bnd > 0, err / bnd.clamp_min(1e-300), torch.full_like(err, float("inf"))))
    ratio = torch.where(torch.isfinite(got.double()), ratio, torch.full_like(ratio, float("inf")))
    ratio = torch.where(err == 0, torch.zeros_like(ratio), ratio)
    flat = int(ratio.argmax())
    idx = []
    for n in reversed(ratio.shape):
        idx.append(flat % n)
        flat //= n
    return float(ratio.max()), tuple(reversed(idx))


def assert_close(got, out, mag, kind, case, limit, roundings=2, what=""):
    """the per-element bound, with a message that names the element and the boundaries next to it"""
    r, (b, h, i, d) = compare(got, out, mag, kind, roundings)
    if r <= 1.0:
        return r
    lim = int(limit[b, i])
    raise AssertionError(
        f"{case.name} {what} [{kind}]: |got - ref| = {r:.3g} x the bound at (batch row {b}, head {h}, query {i}, dim {d}): "
        f"got {float(got[b, h, i, d]):.6g}, ref {float(out[b, h, i, d]):.6g}, mag {float(mag[b, h, i, d]):.3g}; "
        f"q_pos0_b = {case.pos0(b)}, limit = {lim} (limit % 64 = {lim % 64}, key tile {max(lim - 1, 0) // 64}), kvmax_b = {case.kvmax(b)}, "
        f"Skv_b = {case.skv(b)}, query block {i // 128}, wave {(i % 128) // 32}, q-tile row {i % 16}")


def reference(D, case):
    """(out, mag, limit) of the contract for the data of make_case"""
    lim = limits(case)
    out, mag = ref64(D["q_eff"], D["k"], D["v"], visible(lim, case.kv_stride), D["scale"])
    return out, mag, lim


# ------------------------------------------------------------------------------------------------ tile-wise restatement
def tiled(q, k, v, limit, scale, dtype, round_p=None, rescale=True):
    """attention_kernel's algorithm restated in torch: 64-key tiles, a running max in raw score units, exp2 with the folded scale,
    accumulation in `dtype`; round_p rounds P before P.V (the row sum is taken before that); rescale=False is the mutant that
    forgets `o *= alpha`.  -> out [B,H,Lq,hd] in `dtype` (not rounded)."""
    q, k, v = q.to(dtype), k.to(dtype), v.to(dtype)
    B, H, Lq, hd = q.shape
    cs = torch.tensor(scale * 1.4426950408889634, dtype=dtype)
    m_run = torch.full((B, H, Lq, 1), -1e30, dtype=dtype)
    l_run = torch.zeros((B, H, Lq, 1), dtype=dtype)
    o = torch.zeros((B, H, Lq, hd), dtype=dtype)
    for t in range(-(-int(limit.max()) // 64)):
        kt, vt = k[:, :, 64 * t:64 * t + 64], v[:, :, 64 * t:64 * t + 64]
        vis = visible(limit - 64 * t, kt.shape[2])
        s = (q @ kt.transpose(-1, -2)).masked_fill(~vis, -1e30)
        m_new = torch.maximum(m_run, s.amax(-1, keepdim=True))
        alpha = torch.exp2((m_run - m_new) * cs)
        p = torch.exp2(s * cs - m_new * cs) * vis
        l_run = l_run * alpha + p.sum(-1, keepdim=True)
        if rescale:
            o = o * alpha
        o = o + (round_p(p) if round_p else p).to(dtype) @ vt
        m_run = m_new
    return torch.where(l_run > 0, o / torch.where(l_run > 0, l_run, torch.ones_like(l_run)), torch.zeros_like(o))


def emulate(D, case, roundings=True):
    """the fp32 restatement on a case: with the storage's roundings of P and of the output (what a correct kernel may do), or
    without (the fp32 share alone: C32 is measured on this)"""
    kind = D["kind"]
    qe = rotated_q(D, case, torch.float32) if case.fused else D["q"]
    rp = (lambda p: round_kind(p, kind)) if roundings else None
    out = tiled(qe, D["k"], D["v"], limits(case), D["scale"], torch.float32, round_p=rp)
    return round_kind(out, kind) if roundings else out


# ------------------------------------------------------------------------------------------------ mutants (CPU only)
def _masked(case, D, vis2):
    vis = visible(limits(case), case.kv_stride)
    if torch.equal(vis2, vis):
        return None
    return ref64(D["q_eff"], D["k"], D["v"], vis2, D["scale"])[0]


def _limit_mutant(**kw):
    return lambda case, D: _masked(case, D, visible(limits(case, **kw), case.kv_stride))


def _drop_keys(rem):
    def f(case, D):
        j = torch.arange(case.kv_stride)
        drop = (j % 64 == rem) & (j >= 63)
        return _masked(case, D, visible(limits(case), case.kv_stride) & ~drop)
    return f


def _no_rescale(case, D):
    lim = limits(case)
    if int(lim.max()) <= 64:
        return None          # single tile: nothing to rescale
    return tiled(D["q_eff"], D["k"], D["v"], lim, D["scale"], F64, rescale=False)


def _rope_no_pos(case, D):
    if not case.fused or all(case.pos0(b) == 0 for b in range(case.B)):
        return None
    return ref64(rotated_q(D, case, F64, use_pos0=False), D["k"], D["v"], visible(limits(case), case.kv_stride), D["scale"])[0]


def _masked_mean(case, D):
    lim = limits(case)
    if int(lim.min()) > 0:
        return None
    out = ref64(D["q_eff"], D["k"], D["v"], visible(lim, case.kv_stride), D["scale"])[0]
    mean = D["v"].double().mean(2, keepdim=True).expand_as(out)
    return torch.where((lim == 0)[:, None, :, None], mean, out)


def _paged(page_of):
    def f(case, D):
        if not case.paged:
            return None
        kp, vp, table = build_pages(D, case)
        k2, v2 = gather_pages(kp, vp, table, case, page_of)
        k1, v1 = gather_pages(kp, vp, table, case)
        lim = limits(case)
        seen = visible(lim, case.kv_stride).any(2)[:, 0]            # [B, S]: keys some query of the row sees
        if torch.equal(k2[seen[:, None, :].expand(k2.shape[:3])], k1[seen[:, None, :].expand(k1.shape[:3])]):
            return None
        return ref64(D["q_eff"], k2, v2, visible(lim, case.kv_stride), D["scale"])[0]
    return f


def _other_row(case):
    return lambda b, t: ((b ^ 1 if (b ^ 1) < case.B else b), t)


# name -> (function(case, D) -> wrong float64 output, or None where the mutant leaves this case's result unchanged by construction;
#          the profiles in which the comparator must reject it)
MUTANTS = {
    "causal_plus1": (_limit_mutant(causal_off=1), ("recent",)),
    "causal_minus1": (_limit_mutant(causal_off=-1), ("recent",)),
    "kvlen_plus1": (_limit_mutant(kvlen_off=1), ("flat", "recent")),
    "kvlen_minus1": (_limit_mutant(kvlen_off=-1), ("recent",)),
    "skv_plus1": (_limit_mutant(skv_off=1), ("flat", "early")),
    "drop_tile_first_key": (_drop_keys(0), ("recent",)),
    "drop_tile_last_key": (_drop_keys(63), ("recent",)),
    "qtile_plus16": (_limit_mutant(row_shift=16), ("recent",)),
    "qtile_minus16": (_limit_mutant(row_shift=-16), ("recent",)),
    "other_row_kvlen": (_limit_mutant(swap_kvlen=True), ("recent",)),
    "other_row_pos": (_limit_mutant(swap_pos=True), ("recent",)),
    "no_alpha_rescale": (_no_rescale, ("recent",)),
    "rope_without_pos0": (_rope_no_pos, ("flat",)),
    "masked_row_mean_v": (_masked_mean, ("flat",)),
    "page_of_next_tile": (lambda case, D: _paged(lambda b, t: (b, t + 1))(case, D), ("early", "recent")),
    "page_of_other_row": (lambda case, D: _paged(_other_row(case))(case, D), ("recent",)),
}
