"""Grounded decoding, host side (no GPU): groma_amd.grammar against this file's own restatement of the grammar table, the C entry
point's argument validation, evalkit.region_lists, and the argument handling of submit(grounded=True) / generate(grounded=True)."""
import ctypes
import itertools

import pytest
import torch

V = 32114
BOR, EOR, R0, RC, EOS = 32004, 32005, 32014, 100, 2             # the ids of constants.derived_token_ids()
NEVER = (32008, 32009, 32010, 32011, 32012, 32000)               # <image> <region> <refer_box> <ground_box> <refer_feat> [PAD]


# ---- the restatement (state, token -> state; state, n -> allowed set), independent of groma_amd.grammar
def _next(s, t):
    if s < 0 or t is None:
        return s
    return 1 if t == BOR else 2 if R0 <= t < R0 + RC else 0 if t == EOR else s


def _allowed(s, n, t):
    n = max(0, min(n, RC))
    if s < 0:
        return True
    if s == 0:
        return not (R0 <= t < R0 + RC or t == EOR or t in NEVER or (n == 0 and t == BOR))
    return R0 <= t < R0 + n or (t == EOR and (s == 2 or n == 0))


def _violation(new, n, stop=None):
    s = 0
    for i, t in enumerate(new):
        if not _allowed(s, n, t):
            return i
        if t == stop:
            return None
        s = _next(s, t)
    return None


def _ids():
    from groma_amd.grammar import GrammarIds
    return GrammarIds(BOR, EOR, R0, RC, NEVER)


def _token_classes(n):
    """one representative of every token class the table speaks about"""
    return {"none": None, "bor": BOR, "eor": EOR, "r_first": R0, "r_last": R0 + RC - 1, "r_n": R0 + min(n, RC - 1),
            "r_n-1": R0 + max(n - 1, 0), "ordinary": 17, "eos": EOS, "never": NEVER[0], "pad": NEVER[-1], "below_R": R0 - 1,
            "above_R": R0 + RC}


@pytest.mark.parametrize("n", [0, 1, 37, 100])
def test_grammar_module_agrees_with_the_table(n):
    from groma_amd import grammar
    ids = _ids()
    every = torch.arange(V)
    for s in (-1, 0, 1, 2):
        want = torch.tensor([not _allowed(s, n, t) for t in every.tolist()])
        got = grammar.banned_mask(s, n, V, ids)
        assert got.dtype == torch.bool and got.shape == (V,) and torch.equal(got, want), (s, n)
        for name, t in _token_classes(n).items():
            assert grammar.next_state(s, t, ids) == _next(s, t), (s, name)
    assert torch.equal(grammar.banned_mask(1, 250, V, ids), grammar.banned_mask(1, 100, V, ids))   # n is clamped to r_count
    # first_violation: every sequence of three class representatives
    toks = [t for t in _token_classes(n).values() if t is not None]
    for seq in itertools.product(toks, repeat=3):
        assert grammar.first_violation(list(seq), n, ids) == _violation(seq, n), (seq, n)
        assert grammar.first_violation(torch.tensor(seq), n, ids, stop=EOS) == _violation(seq, n, EOS), (seq, n)


def test_grammar_consequences():
    """what the docstring promises: EOS only in TEXT, k < n, lists non-empty, a cut list shows in the final state"""
    from groma_amd import grammar
    ids = _ids()
    for n in (1, 37, 100):
        assert bool(grammar.banned_mask(1, n, V, ids)[EOS]) and bool(grammar.banned_mask(2, n, V, ids)[EOS])
        assert not bool(grammar.banned_mask(0, n, V, ids)[EOS])
        assert bool(grammar.banned_mask(1, n, V, ids)[EOR]) and not bool(grammar.banned_mask(2, n, V, ids)[EOR])
        for s in (1, 2):
            m = grammar.banned_mask(s, n, V, ids)
            assert not bool(m[R0: R0 + n].any()) and bool(m[R0 + n: R0 + RC].all())
    assert grammar.final_state([5, BOR, R0], ids) == 2 and grammar.final_state([5, BOR], ids) == 1
    assert grammar.final_state([5, BOR, R0, EOR, EOS], ids) == 0
    assert grammar.first_violation([5, BOR, R0 + 2, R0, EOR, 9, EOS, NEVER[-1], NEVER[-1]], 3, ids, stop=EOS) is None
    assert grammar.first_violation([5, BOR, R0 + 3], 3, ids) == 2          # <r_3> with three boxes
    assert grammar.first_violation([5, BOR, EOR], 3, ids) == 2             # an empty list
    assert grammar.first_violation([5, BOR, R0, EOS], 3, ids) == 3         # EOS inside a list
    assert grammar.first_violation([5, R0], 3, ids) == 1                   # <r_k> in running text
    assert grammar.first_violation([BOR], 0, ids) == 0                     # no boxes: no list


def test_ids_from_model():
    from groma_amd import constants, grammar
    from tests import util
    tk = util.TokenIds()
    with pytest.raises(ValueError):                                         # <roi> / </roi> unknown
        grammar.GrammarIds.from_model(tk)
    cv = constants.SyntheticTokenizer().convert_tokens_to_ids
    tk.bor_token_id, tk.eor_token_id = cv(["<roi>", "</roi>"])
    ids = grammar.GrammarIds.from_model(tk)
    assert (ids.bor, ids.eor) == tuple(cv(["<roi>", "</roi>"])) and ids.r_first == tk.box_idx_token_ids[0] and ids.r_count == 100
    assert set(ids.never) == {tk.img_token_id, tk.reg_token_id, tk.refer_box_token_id, tk.ground_box_token_id,
                              tk.refer_feat_token_id, tk.pad_token_id} and len(ids.never) <= 8
    tk.box_idx_token_ids = tk.box_idx_token_ids[:50] + [x + 1 for x in tk.box_idx_token_ids[50:]]
    with pytest.raises(ValueError, match="contiguous"):
        grammar.GrammarIds.from_model(tk)


def test_model_learns_the_brackets_from_the_tokenizer():
    from groma_amd import constants
    from groma_amd.groma import GromaModel
    m = GromaModel.__new__(GromaModel)
    m.generation_config = type("GC", (), {})()
    tk = constants.SyntheticTokenizer()
    m.init_special_token_id(tk)
    assert [m.bor_token_id, m.eor_token_id] == tk.convert_tokens_to_ids(["<roi>", "</roi>"])


def test_symbol_is_exported_by_all_three_builds():
    from groma_amd import _lib
    from groma_amd.csrc import build as hip_build
    hip_build.build(verbose=False)                                       # (compiles only what is stale)
    assert "gr_grammar_step" in _lib.SIGNATURES
    for path in (_lib.LIB_PATH, _lib.LIB_PATH_F16, _lib.LIB_PATH_REF):
        assert hasattr(ctypes.CDLL(path), "gr_grammar_step"), path
    assert _lib.load().gr_abi_version() == 9


def test_bad_arguments_are_rejected_without_a_gpu():
    from groma_amd import _lib
    P = ctypes.c_void_p
    nv = (ctypes.c_long * 8)(*range(10, 18))
    ok = dict(logits=P(64), rows=4, V=300, ld=320, state=P(64), last_tok=None, n_boxes=P(64), r_first=150, r_count=100, bor=8,
              eor=9, never=nv, n_never=4)
    bad = [dict(logits=None), dict(state=None), dict(n_boxes=None), dict(rows=0), dict(rows=-1), dict(V=0), dict(ld=299),
           dict(r_count=-1), dict(n_never=9), dict(n_never=2, never=None), dict(r_first=-1), dict(r_first=201), dict(r_first=300, r_count=1),
           dict(bor=300), dict(bor=-1), dict(eor=300), dict(eor=-1), dict(eor=8), dict(bor=150), dict(eor=249),
           dict(never=(ctypes.c_long * 8)(10, 300, 12, 13, 0, 0, 0, 0)), dict(never=(ctypes.c_long * 8)(-1, 11, 12, 13, 0, 0, 0, 0))]
    for name in ("bf16", "fp16", "ref"):
        lib = _lib.load(name)
        for b in bad:
            a = dict(ok, **b)
            assert lib.gr_grammar_step(*a.values(), None) == 22, (name, b)


def test_region_lists():
    from groma_amd.evalkit import region_lists
    box = list(range(R0, R0 + RC))
    r = lambda k: R0 + k
    assert region_lists([5, 6, 7], box, BOR, EOR) == []
    assert region_lists([5, BOR, r(3), EOR, 6, BOR, r(0), r(99), r(3), EOR, EOS], box, BOR, EOR) == [[3], [0, 99, 3]]
    assert region_lists(torch.tensor([BOR, r(1), r(2)]), box, BOR, EOR) == [[1, 2]]            # cut open by the end of the answer
    assert region_lists([BOR], box, BOR, EOR) == [[]]
    assert region_lists([r(4), BOR, r(5), 17, EOR, r(6), EOR], box, BOR, EOR) == [[5]]         # <r_k> in running text is not a list
    assert region_lists([BOR, r(1), BOR, r(2), EOR], box, BOR, EOR) == [[1], [2]]              # a second <roi> closes the first
    shuffled = [R0 + 2 * k for k in range(50)]                                                  # a non-contiguous vocabulary
    assert region_lists([BOR, R0 + 4, R0 + 5, EOR], shuffled, BOR, EOR) == [[2]]


def test_submit_and_generate_argument_handling():
    """what needs no device: submit(grounded=True) on a batcher built without the flag, the Request fields, a grounded row count"""
    from groma_amd import serving
    from groma_amd.groma import GromaModel
    b = serving.ContinuousBatcher.__new__(serving.ContinuousBatcher)
    b.grounded, b.queue, b.live, b._next_rid = False, [], {}, 0
    b.model = type("M", (), {"generation_config": type("GC", (), {"eos_token_id": None})()})()
    with pytest.raises(ValueError, match="grounded"):
        b.submit(torch.tensor([1, 2, 3]), None, grounded=True)
    assert not b.queue
    rid = b.submit(torch.tensor([1, 2, 3]), None)
    assert b.live[rid].grounded is False and b.live[rid].grammar_state is None
    b.grounded = True
    rid = b.submit(torch.tensor([1, 2, 3]), None, grounded=True, logprobs=2)
    assert b.live[rid].grounded is True and b.live[rid].logprobs_k == 2
    m = GromaModel.__new__(GromaModel)
    m.generation_config = type("GC", (), {})()
    with pytest.raises(ValueError, match="one entry per row"):
        m._generate(torch.zeros((2, 4), dtype=torch.int64), grounded=[True])
    with pytest.raises(ValueError, match="init_special_token_id"):      # the ids are not known
        m._generate(torch.zeros((2, 4), dtype=torch.int64), grounded=True)
