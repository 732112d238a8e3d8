"""CPU checks of tests/row_cases.py (the fixtures of tests/test_vision_rows_gpu.py), per operation: the float64 reference agrees with
torch's own float64 statement of the operation; the comparator is sound (the fp32 restatement of the kernel, with the storage's output
rounding, passes it with ratio <= 1 on every case and storage); its fp32 constant is the measured one (printed next to the recorded
value; the test fails when the record goes stale); it bites (every mutant is rejected with a factor >= 2 on every case it applies
to, and a mutant made a no-op is noticed); and the case lists hold the edges they are meant to hold."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests import row_cases as R

F64, F32 = torch.float64, torch.float32
OUT_KINDS = R.KINDS + (None,)


# ------------------------------------------------------------------------------------------------ shared references (computed once)
@functools.lru_cache(maxsize=None)
def _norm(name):
    c = {c.name: c for c in R.NORM_CASES}[name]
    D = R.make_norm(c)
    return c, D, R.norm_ref64(c, D)


@functools.lru_cache(maxsize=None)
def _gn(name, kind):
    c = {c.name: c for c in R.GN_CASES}[name]
    D = R.make_gn(c, kind)
    return c, D, R.gn_ref64(c, D)


@functools.lru_cache(maxsize=None)
def _shuf(name, kind):
    c = {c.name: c for c in R.SHUF_CASES}[name]
    D = R.make_shuf(c, kind)
    return c, D, R.shuf_eval(c, D, F64, want_mag=True)


@functools.lru_cache(maxsize=None)
def _up(name):
    c = {c.name: c for c in R.UP_CASES}[name]
    D = R.make_up(c)
    return c, D, R.up_eval(c, D, F64, want_mag=True)


@functools.lru_cache(maxsize=None)
def _msda(name):
    c = {c.name: c for c in R.MSDA_CASES}[name]
    D = R.make_msda(c)
    return c, D, R.msda_eval(c, D, F64, want="mag")


def test_case_names_are_unique():
    for lst in (R.NORM_CASES, R.GN_CASES, R.SHUF_CASES, R.UP_CASES, R.MSDA_CASES):
        assert len({c.name for c in lst}) == len(lst)


# ------------------------------------------------------------------------------------------------ the references against torch's own
def test_norm_reference_is_torch_layer_norm():
    for case in R.NORM_CASES:
        c, D, (ref, mag) = _norm(case.name)
        v = D["x"].double() + (D["add"].double() if c.add else 0.0)
        v = v.clamp_min(0.0) if c.relu else v
        if c.op == "ln":
            want = F.layer_norm(v, (c.C,), D["gamma"].double(), D["beta"].double() if c.beta else None, c.eps)
        else:
            want = D["gamma"].double() * v * torch.rsqrt(v.pow(2).mean(-1, keepdim=True) + c.eps)
        assert float((ref - want).abs().max()) <= 1e-12 * float(mag.max())
        assert bool((mag >= ref.abs() * (1 - 1e-12)).all())
        if c.profile == "const":      # the constant row: the reference IS beta (0 without one), eps the whole denominator
            r = c.rows // 2
            want_row = D["beta"].double() if c.beta else torch.zeros(c.C, dtype=F64)
            if c.op == "ln":
                assert float((ref[r] - want_row).abs().max()) <= 1e-9


def test_gn_reference_is_torch_group_norm():
    for case in R.GN_CASES:
        c, D, ref = _gn(case.name, "bf16")
        x = D["x"].double().permute(0, 2, 1).reshape(R.GN_IMGS, R.GN_C, c.HW, 1)
        want = F.group_norm(x, c.groups, D["gamma"].double(), D["beta"].double(), R.GN_EPS)
        mine = x * ref["a"].view(R.GN_IMGS, R.GN_C, 1, 1) + ref["b"].view(R.GN_IMGS, R.GN_C, 1, 1)
        assert float((mine - want).abs().max()) <= 1e-9 * (1 + c.R) ** 2
        ratio = (ref["mean"].abs() / ref["var"].sqrt())
        assert c.R * 0.75 <= float(ratio.min()) and float(ratio.max()) <= c.R * 1.4 + 0.5, (c.name, float(ratio.min()), float(ratio.max()))
        per_ch = D["x"].double().mean(1)            # the channel means differ inside the groups (bf16's grid at 32 is 0.25 wide: nearly all)
        assert float(((per_ch[:, 0::2] - per_ch[:, 1::2]).abs() > 0).double().mean()) > 0.9 and float((per_ch[0] - per_ch[1]).abs().min()) > 0


def test_resize_reference_is_torch_interpolate():
    g = torch.Generator().manual_seed(5)
    for Ss, S in ((6, 12), (12, 6), (3, 6), (5, 10), (10, 5), (5, 3), (6, 24), (5, 7), (4, 9), (3, 1), (6, 6)):
        src = torch.randn((2, Ss, Ss, 8), generator=g, dtype=F64)
        got, _ = R._resize_ac(src, None, S, F64)
        want = F.interpolate(src.permute(0, 3, 1, 2), size=(S, S), mode="bilinear", align_corners=True).permute(0, 2, 3, 1)
        assert float((got - want).abs().max()) <= 1e-12, (Ss, S)


def test_shuffle_reference_is_the_reference_model_statement():
    """relu(gn(.)) per source, the channel shuffle of the three levels, bilinear align_corners=True to the target size -- with torch's
    own interpolate"""
    C = R.SHUF_C
    for case in R.SHUF_CASES:
        c, D, (ref, mag) = _shuf(case.name, "fp16")

        def act(lvl, use):
            x = D["maps"][lvl].double()
            if not use:
                return x
            cf = D["coef"][lvl].double()
            return F.relu(x * cf[:, 0].view(2, 1, 1, C) + cf[:, 1].view(2, 1, 1, C))

        def rs(t):
            return F.interpolate(t.permute(0, 3, 1, 2), size=(c.S, c.S), mode="bilinear", align_corners=True).permute(0, 2, 3, 1)

        if c.shuffle:
            want = torch.cat([act(c.lvl, c.coef[0])[..., :C // 2], rs(act(c.top, c.coef[1])[..., 3 * C // 4:]),
                              rs(act(c.down, c.coef[2])[..., C // 2:3 * C // 4])], -1)
        else:
            want = act(c.lvl, c.coef[0])
        assert float((ref - want).abs().max()) <= 1e-12
        assert bool((mag >= ref.abs() * (1 - 1e-12)).all())


def test_msda_reference_is_grid_sample():
    """the direct statement against mmcv's multi_scale_deformable_attn_pytorch form: grid_sample(bilinear, zeros, align_corners=False)"""
    for case in R.MSDA_CASES:
        c, D, (ref, mag) = _msda(case.name)
        B, Q, H, P = R.MSDA_B, R.MSDA_Q, c.heads, R.MSDA_P
        off = D["offw"][:, :H * P * 2].double().view(B, Q, H, P, 2)
        aw = torch.softmax(D["offw"][:, H * P * 2:c.n].double().view(B, Q, H, P), -1)
        r = D["ref"].double()
        r = r.view(B, Q, 1, 1, c.rdim) if c.ref_batched else r.view(1, Q, 1, 1, c.rdim).expand(B, Q, 1, 1, c.rdim)
        loc = r[..., :2] + (off / torch.tensor([c.Ws, c.Hs], dtype=F64) if c.rdim == 2 else off / P * r[..., 2:] * 0.5)
        v = D["value"].double().flatten(2).transpose(1, 2).reshape(B * H, R.MSDA_D, c.Hs, c.Ws)
        samp = F.grid_sample(v, (2 * loc - 1).transpose(1, 2).flatten(0, 1), mode="bilinear", padding_mode="zeros", align_corners=False)
        want = (samp * aw.transpose(1, 2).reshape(B * H, 1, Q, P)).sum(-1).view(B, H * R.MSDA_D, Q).transpose(1, 2).reshape(B * Q, -1)
        assert float((ref - want).abs().max()) <= 1e-12
        assert bool((mag >= ref.abs() * (1 - 1e-12)).all())


def test_linspace_restatement():
    """the kernel's two-sided form with contracted multiply-adds gives torch.linspace's bits"""
    for n in sorted({c.Ho for c in R.UP_CASES} | {16, 32, 48, 64}):
        assert torch.equal(R.linspace_two_sided(n), torch.linspace(-1, 1, n)), n


def test_e4m3_table_and_rounding():
    assert len(R.E4M3_GRID) == 253 and float(R.E4M3_GRID.max()) == 448.0 and float(R.E4M3_GRID.min()) == -448.0
    assert float(R.E4M3[0x38]) == 1.0 and float(R.E4M3[0x01]) == 2.0 ** -9 and float(R.E4M3[0xfe]) == -448.0
    if hasattr(torch, "float8_e4m3fn"):
        t = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).float().double()
        ok = torch.isfinite(R.E4M3)
        assert torch.equal(t[ok], R.E4M3[ok]) and bool(torch.isnan(t[~ok]).all())
        x = torch.randn(20000, generator=torch.Generator().manual_seed(1), dtype=F64).mul(120).clamp(-448, 448).float()
        assert torch.equal(x.to(torch.float8_e4m3fn).float().double(), R.e4m3_round(x.double()))
    x = torch.tensor([0.0, 1.0, 1.06, 1.0625, 1.1875, 447.0, 448.0, -500.0], dtype=F64)
    assert R.e4m3_round(x.clamp(-448, 448)).tolist() == [0.0, 1.0, 1.0, 1.0, 1.25, 448.0, 448.0, -448.0]


# ------------------------------------------------------------------------------------------------ sound: the restatements pass
def _norm_ratio(case, got, kind):
    c, D, (ref, mag) = _norm(case.name)
    return R.norm_compare(got, ref, mag, kind, c)[0]


def test_norm_restatement_within_bound():
    for case in R.NORM_CASES:
        c, D, _ = _norm(case.name)
        got = R.norm_restate(c, D)
        for kind in OUT_KINDS:
            if kind is not None and not c.out16:
                continue
            r = _norm_ratio(c, got if kind is None else R.round_kind(got, kind), kind)
            assert r <= 1.0, (c.name, kind, r)


def test_gn_restatement_within_bound():
    for case in R.GN_CASES:
        for kind in R.KINDS:
            c, D, ref = _gn(case.name, kind)
            r, idx = R.gn_compare(R.gn_restate(c, D)[0], ref, D)
            assert r <= 1.0, (c.name, kind, r, idx)


def test_shuffle_restatement_within_bound():
    q = R.SHUF_Q_INV
    for case in R.SHUF_CASES:
        for kind in R.KINDS:
            c, D, (ref, mag) = _shuf(case.name, kind)
            got, _ = R.shuf_eval(c, D, F32)
            r = R.compare(R.round_kind(got, kind), ref, mag, kind, "shuffle")[0]
            assert r <= 1.0, (c.name, kind, r)
            if kind != "ref":       # st8q: the fp32 product with q_inv, clamped, rounded to nearest even
                byte = R.e4m3_round((got * torch.tensor(q)).double().clamp(-448.0, 448.0))
                rq, idx = R.shuf_compare_q8(byte, ref, mag, q)
                assert rq <= 1.0, (c.name, kind, rq, idx)


def test_upsample_restatement_within_bound():
    for case in R.UP_CASES:
        c, D, (ref, mag) = _up(case.name)
        got, _ = R.up_eval(c, D, F32)
        for kind in R.KINDS:
            r, idx = R.up_compare(R.round_kind(got, kind), ref, mag, kind, c)
            assert r <= 1.0, (c.name, kind, r, idx)


def test_msda_restatement_within_bound():
    for case in R.MSDA_CASES:
        c, D, (ref, mag) = _msda(case.name)
        r, idx = R.msda_compare(R.msda_eval(c, D, F32), ref, mag)
        assert r <= 1.0, (c.name, r, idx)


# ------------------------------------------------------------------------------------------------ the constants are the measured ones
def _measure():
    m = {"ln": 0.0, "rms": 0.0, "shuffle": 0.0, "upsample": 0.0, "msda": 0.0}
    for case in R.NORM_CASES:
        c, D, (ref, mag) = _norm(case.name)
        m[c.op] = max(m[c.op], float(((R.norm_restate(c, D).double() - ref).abs() / mag).max()))
    for case in R.SHUF_CASES:
        for kind in R.KINDS:
            c, D, (ref, mag) = _shuf(case.name, kind)
            m["shuffle"] = max(m["shuffle"], float(((R.shuf_eval(c, D, F32)[0].double() - ref).abs() / mag).max()))
    for case in R.UP_CASES:
        c, D, (ref, mag) = _up(case.name)
        err = (R.up_eval(c, D, F32)[0][..., :R.UP_C].double() - ref[..., :R.UP_C]).abs()
        m["upsample"] = max(m["upsample"], float((err / mag).max()))
    for case in R.MSDA_CASES:
        c, D, (ref, mag) = _msda(case.name)
        m["msda"] = max(m["msda"], float(((R.msda_eval(c, D, F32).double() - ref).abs() / mag).max()))
    return m


def test_c32_measured():
    """C32[op] = C32_FACTOR x the fp32 share measured here: the restatement WITHOUT 16-bit roundings against float64, over the op's whole
    case list.  The record may exceed the measurement by a rounding-up only."""
    m = _measure()
    for op, v in m.items():
        print(f"{op:9s} worst |restatement - ref64| / mag = {v:.3e}; recorded C32_MEASURED = {R.C32_MEASURED[op]:.3e}, C32 = {R.C32[op]:.3e}")
    for op, v in m.items():
        assert 0.8 * R.C32_MEASURED[op] <= v <= R.C32_MEASURED[op], f"{op}: measured {v:.3e}: update C32_MEASURED in tests/row_cases.py"
        assert R.C32[op] == R.C32_FACTOR * R.C32_MEASURED[op]
    assert R.C32_FACTOR == 4
    # the fp32 share stays a small part of the 16-bit storages' unit roundoff wherever mag is of the order of |ref|
    assert max(R.C32.values()) < 0.01 * R.U["bf16"] and max(R.C32.values()) < 0.01 * R.U["fp16"] * 8


def test_c_gn_measured():
    """the restated rstd's worst relative error in units of 2^-24 (1 + mean^2 / (var + eps)), per |mean| / std class and overall"""
    by_r = {r: 0.0 for r in R.GN_RATIOS}
    for case in R.GN_CASES:
        for kind in R.KINDS:
            c, D, ref = _gn(case.name, kind)
            rstd = R.gn_restate(c, D)[1].double()
            true = 1.0 / torch.sqrt(ref["var"] + R.GN_EPS)
            unit = R.EPS24 * (1.0 + ref["mean"] ** 2 / (ref["var"] + R.GN_EPS))
            by_r[c.R] = max(by_r[c.R], float(((rstd - true).abs() / true / unit).max()))
    worst = max(by_r.values())
    print(f"rstd error in units of 2^-24 (1 + mean^2 / var) by |mean| / std: {by_r}; worst {worst:.3f}; recorded C_GN_MEASURED = "
          f"{R.C_GN_MEASURED}, C_GN = {R.C_GN}")
    assert 0.8 * R.C_GN_MEASURED <= worst <= R.C_GN_MEASURED, f"measured {worst:.3f}: update C_GN_MEASURED in tests/row_cases.py"
    assert R.C_GN == 4 * R.C_GN_MEASURED and R.C_GN_FACTOR == 4
    # the contract as stated in row_cases.py and include/groma_hip.h: a's relative error below a sixteenth of the map's output rounding
    assert R.C_GN * R.EPS24 * (1 + 16.0 ** 2) <= R.U["bf16"] / 16 and R.C_GN * R.EPS24 * (1 + 5.6 ** 2) <= R.U["fp16"] / 16


# ------------------------------------------------------------------------------------------------ biting: the mutants
def _norm_verdicts(name):
    kw, applies = R.NORM_MUTANTS[name]
    rows = []
    for case in R.NORM_CASES:
        if applies(case):
            c, D, (ref, mag) = _norm(case.name)
            rows.append((c.name, "f32", R.norm_compare(R.norm_restate(c, D, **kw), ref, mag, None, c)[0]))
    return rows


def _gn_verdicts(name):
    kw, applies = R.GN_MUTANTS[name]
    rows = []
    for case in R.GN_CASES:
        if applies(case):
            c, D, ref = _gn(case.name, "bf16")
            rows.append((c.name, "bf16", R.gn_compare(R.gn_restate(c, D, **kw)[0], ref, D)[0]))
    return rows


def _shuf_verdicts(name):
    rows = []
    for case in R.SHUF_CASES:
        if R.shuf_applies(name, case):
            c, D, (ref, mag) = _shuf(case.name, "bf16")
            rows.append((c.name, "bf16", R.compare(R.shuf_eval(c, D, F32, **R.SHUF_MUTANTS[name])[0], ref, mag, "bf16", "shuffle")[0]))
    return rows


def _up_verdicts(name):
    kw, applies, kinds = R.UP_MUTANTS[name]
    rows = []
    for case in R.UP_CASES:
        if applies(case):
            c, D, (ref, mag) = _up(case.name)
            got = R.up_eval(c, D, F32, **kw)[0]
            rows += [(c.name, kind, R.up_compare(R.round_kind(got, kind), ref, mag, kind, c)[0]) for kind in kinds]
    return rows


def _msda_verdicts(name):
    kw, applies = R.MSDA_MUTANTS[name]
    rows = []
    for case in R.MSDA_CASES:
        if applies(case):
            c, D, (ref, mag) = _msda(case.name)
            rows.append((c.name, "f32", R.msda_compare(R.msda_eval(c, D, F32, **kw), ref, mag)[0]))
    return rows


FAMILIES = {"norm": (R.NORM_MUTANTS, _norm_verdicts), "gn": (R.GN_MUTANTS, _gn_verdicts), "shuffle": (R.SHUF_MUTANTS, _shuf_verdicts),
            "upsample": (R.UP_MUTANTS, _up_verdicts), "msda": (R.MSDA_MUTANTS, _msda_verdicts)}


@pytest.mark.parametrize("family,name", [(f, n) for f, (muts, _) in FAMILIES.items() for n in muts])
def test_comparator_rejects_mutant(family, name):
    rows = FAMILIES[family][1](name)
    assert len({r[0] for r in rows}) >= 2, f"{name} applies to {sorted({r[0] for r in rows})}: a mutant must apply to at least two cases"
    print(f"{family}/{name}: {len(rows)} verdicts, weakest {min(r[2] for r in rows):.3g}")
    for case, kind, r in rows:
        assert r >= 2.0, f"{name} on {case} [{kind}]: only {r:.3g} x the bound -- the comparator would accept this kernel"


def test_mutant_lists_are_the_issue_s():
    assert [len(FAMILIES[f][0]) for f in ("norm", "gn", "shuffle", "upsample", "msda")] == [8, 6, 7, 4, 7]


@pytest.mark.parametrize("family,name,noop", [("norm", "divisor_c_minus_1", (dict(divisor="C"), lambda c: True)),
                                              ("gn", "image_index_ignored", (dict(ignore_img=False), lambda c: True)),
                                              ("shuffle", "top_down_swapped", dict(swap_src=False)),
                                              ("upsample", "cls_skip_missing", (dict(no_cls_skip=False), lambda c: True, ("bf16", "ref"))),
                                              ("msda", "hs_ws_swapped", (dict(swap_hw=False), lambda c: True))])
def test_a_noop_mutant_is_noticed(monkeypatch, family, name, noop):
    """the sensitivity test fails when a mutant is made a no-op"""
    monkeypatch.setitem(FAMILIES[family][0], name, noop)
    with pytest.raises(AssertionError):
        test_comparator_rejects_mutant(family, name)


def test_q8_comparator_bites():
    """the e4m3 bracket rule: a value one grid step outside the bracket, anything but +-448 beyond the clamp, a NaN byte and the
    wrong sign are each rejected; both bracketing values are accepted"""
    c, D, (ref, mag) = _shuf("shuf_12_6_3_l0_c000_p0", "bf16")
    q = R.SHUF_Q_INV
    t = (ref * q).clamp(-448.0, 448.0)
    lo, hi = R.e4m3_floor(t), R.e4m3_ceil(t)
    assert R.shuf_compare_q8(lo, ref, mag, q)[0] <= 1.0 and R.shuf_compare_q8(hi, ref, mag, q)[0] <= 1.0
    beyond = (ref * q).abs() > 448.0 * 1.01
    assert bool(beyond.any()) and bool(((ref * q) > 448.0).any()) and bool(((ref * q) < -448.0).any())
    below = R.e4m3_floor(lo - 1e-9)
    for wrong in (torch.where(beyond, torch.full_like(t, 416.0) * torch.sign(t), lo), torch.where(lo > -448.0, below, lo),
                  torch.where(t.abs() > 1.0, -lo, lo), torch.where(beyond, torch.full_like(t, float("nan")), lo)):
        assert R.shuf_compare_q8(wrong, ref, mag, q)[0] >= 2.0


# ------------------------------------------------------------------------------------------------ coverage of the case lists
def test_norm_coverage():
    C = R.NORM_CASES

    def some(pred, what):
        assert any(pred(c) for c in C), f"no norm case with {what}"

    for op in ("ln", "rms"):
        for width in R.NORM_C_REG + R.NORM_C_GEN:
            for prof in R.NORM_PROFILES:
                if not (op == "rms" and prof == "relu"):
                    some(lambda c: (c.op, c.C, c.profile) == (op, width, prof), f"{op} C={width} {prof}")
            some(lambda c: c.op == op and c.C == width and c.pitched, f"{op} C={width} pitched")
            some(lambda c: c.op == op and c.C == width and not c.pitched, f"{op} C={width} tight")
        for rows in (1, 5, 37):     # 4 rows per block: a block with one row, a partial second block, a partial tenth
            some(lambda c: c.op == op and c.rows == rows and c.fast, f"{op} rows={rows} on the register path")
            some(lambda c: c.op == op and c.rows == rows and not c.fast, f"{op} rows={rows} on the generic path")
    assert {c.C for c in C if c.fast} == set(R.NORM_C_REG) and {c.C for c in C if not c.fast} == set(R.NORM_C_GEN)
    assert {c.C // 256 for c in C if c.fast} == {1, 2, 4, 8, 16}                       # every NV instantiation
    assert any(c.C % 256 == 0 and c.C > 4096 for c in C) and any(c.C % 256 == 0 and (c.C // 256) & (c.C // 256 - 1) for c in C)
    for width in R.NORM_C_REG + R.NORM_C_GEN:
        some(lambda c: c.op == "ln" and c.C == width and c.add, f"C={width} with add")
        some(lambda c: c.op == "ln" and c.C == width and not c.add, f"C={width} without add")
    some(lambda c: c.op == "ln" and not c.beta and c.fast, "beta null on the register path")
    some(lambda c: c.op == "ln" and not c.beta and not c.fast, "beta null on the generic path")
    some(lambda c: c.relu and c.add and c.pitched, "relu_in with add on pitched rows")
    some(lambda c: c.add and c.pitched and c.fast and c.rows > 1, "add sharing ldx on the register path")
    some(lambda c: c.add and c.pitched and not c.fast and c.rows > 1, "add sharing ldx on the generic path")
    assert all(c.ldx % 4 == 0 and c.ldo % 4 == 0 and (not c.out16 or c.ldo % 32 == 0) for c in C)
    assert all(c.out16 == (c.C != 100) for c in C)
    for c in C:
        if c.profile == "mean50":
            _, D, _ = _norm(c.name)
            v = D["x"].double() + (D["add"].double() if c.add else 0.0)
            assert 40 <= float((v.mean(-1) / v.std(-1)).min()) and c.rows == 37
        if c.profile == "relu":
            _, D, _ = _norm(c.name)
            assert c.relu and float((D["x"] < 0).float().mean()) > 0.5


def test_gn_coverage():
    C = R.GN_CASES
    assert {(c.HW, c.groups, c.R) for c in C} == {(h, g, r) for h in R.GN_HW for g in R.GN_GROUPS for r in R.GN_RATIOS}
    assert any(c.nblk == 1 and c.HW % 32 != 0 for c in C), "one block, rows no multiple of the 32 row lanes"
    assert any(c.HW == R.GN_ROWS_PER_BLOCK for c in C), "exactly one block"
    assert any(c.nblk == 2 and 0 < c.HW - R.GN_ROWS_PER_BLOCK < 32 for c in C), "a second block with fewer rows than row lanes"
    assert any(c.nblk >= 3 and (c.HW % R.GN_ROWS_PER_BLOCK) % 32 != 0 for c in C), "three blocks, a clamped last one"
    assert {c.cpg for c in C} == {2, 16, 128}
    assert any(c.nblk * c.cpg > 64 and c.nblk == 1 for c in C), "the finalize loop over more than 64 partials of one block"
    assert any(c.nblk * c.cpg % 64 for c in C if c.nblk > 1), "several blocks whose partials do not fill the finalize lanes"
    assert any(c.cpg > 64 for c in C) and max(c.nblk * c.cpg for c in C) == 384, "more than 64 channels per group"
    assert any(c.nblk * c.cpg < 64 for c in C), "finalize lanes without a partial"
    for c in C:     # the fixture's sums buffer has the kernel's shape
        assert R.gn_partials(c, R.make_gn(c, "bf16")).shape == (R.GN_IMGS, c.nblk, R.GN_C, 2)
        break


def test_gn_fixture_second_variant_keeps_image_1():
    c = R.GN_CASES[0]
    a, b = R.make_gn(c, "fp16"), R.make_gn(c, "fp16", variant=1)
    assert torch.equal(a["x"][1], b["x"][1]) and not torch.equal(a["x"][0], b["x"][0])


def test_shuffle_coverage():
    C = R.SHUF_CASES
    assert {c.sizes for c in C} == set(R.SHUF_SIZES)
    for sizes in R.SHUF_SIZES:
        assert {c.lvl for c in C if c.sizes == sizes and c.shuffle} == {0, 1, 2}        # each level a target
    sh = [c for c in C if c.shuffle]
    assert any(c.sizes[c.top] < c.S for c in sh) and any(c.sizes[c.down] > c.S for c in sh)     # up- and down-scaling
    assert any(c.sizes[c.top] == c.S for c in sh) and any(c.sizes[c.down] == c.S for c in sh)   # the Ss == S branch, either source
    assert any((c.sizes[c.down] - 1) % (c.S - 1) for c in sh) and any((c.S - 1) % max(c.sizes[c.top] - 1, 1) for c in sh)  # fractional
    for role in range(3):
        assert {c.coef[role] for c in sh} == {0, 1}
    assert {c.pad for c in sh} == {0, 1} and any(not c.shuffle for c in C) and {c.coef[0] for c in C if not c.shuffle} == {0, 1}
    q = R.SHUF_Q_INV
    for c in C:     # e4m3: beyond the clamp upwards everywhere, downwards wherever a raw map is a source
        _, D, (ref, mag) = _shuf(c.name, "bf16")
        assert bool((ref * q > 448.0).any()) and bool(((ref * q).abs() < 400.0).any())
        raw = not c.coef[0] or (c.shuffle and not (c.coef[1] and c.coef[2]))
        assert bool((ref * q < -448.0).any()) == raw, c.name


def test_upsample_coverage():
    assert [(c.G, c.Ho) for c in R.UP_CASES] == list(R.UP_CASES_GH)
    assert any(c.Ho == c.G for c in R.UP_CASES) and any(c.Ho % 2 == 1 and c.Ho > 1 for c in R.UP_CASES) and any(c.Ho == 1 for c in R.UP_CASES)
    assert R.UP_CPAD == R.UP_C + 32
    for c in R.UP_CASES:
        _, D, (ref, mag) = _up(c.name)
        assert bool(torch.isnan(D["h"][:, 0]).all()) and bool(torch.isfinite(ref).all()), "the CLS sentinel never reaches the reference"
        if c.Ho > 2:    # x and y channels are told apart on a non-symmetric position
            assert float(ref[0, 0, 1, R.UP_C]) != float(ref[0, 0, 1, R.UP_C + 1]) and float(ref[0, 0, 1, R.UP_C]) == float(ref[0, 1, 0, R.UP_C + 1])


def test_msda_position_classes_are_covered():
    """every case lands samples in every position class: interior, the four one-tap bands, the four corner bands, outside on each side"""
    assert len(R.MSDA_CLASSES) == 13
    for c in R.MSDA_CASES:
        _, D, _ = _msda(c.name)
        got = R.msda_eval(c, D, F64, want="classes")
        assert got == set(R.MSDA_CLASSES), (c.name, set(R.MSDA_CLASSES) - got)
        assert c.Hs != c.Ws and c.ld == c.heads * R.MSDA_P * 3 + 8
        lg = D["offw"][:, c.heads * R.MSDA_P * 2:c.n]
        assert float(lg.max()) > 35.0 and float(D["offw"][:, c.n:].min()) == R.MSDA_CANARY
    assert {(c.heads, c.Hs, c.Ws, c.rdim, c.ref_batched) for c in R.MSDA_CASES} == \
        {(h, a, b, r, rb) for h in (8, 3) for a, b in ((5, 9), (9, 5)) for r in (2, 4) for rb in (0, 1)}
