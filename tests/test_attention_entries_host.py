"""The argument contract of the prefill / decode attention and QKV-split entry points, checked on the host (no GPU).

Every entry validates its arguments before it touches the device and answers 22 (GR_EINVAL) to a bad one.  Each case below takes a
fully valid argument set and breaks exactly one argument.  The valid set itself is the control: without a device the launch fails
with a HIP error code, neither 0 nor 22, which shows that the 22s of the table come from the validation and not from the missing
device.  (gr_attention_bf16 / gr_attention_paged raise the kernels' LDS limit before they launch and answer 22 when that fails, so
they have no such control.)

The module is skipped where a GPU is present: a launcher that let a bad argument through must never launch with it.
"""
import pytest
import torch

if torch.cuda.is_available():
    pytest.skip("host-only: invalid arguments are never sent to a machine that could launch them", allow_module_level=True)

from groma_amd import _lib

P = 0x10000  # a non-null "pointer": validation never dereferences, and no launch can succeed without a device
EINVAL = 22
DEC_SMAX, KV_PAGE = 8192, 64

# entry -> (argument names in ABI order, one valid argument set)
ENTRIES = {
    "gr_attention_bf16": (
        "q k vt out kv_len B H Lq Skv kv_stride head_dim causal q_pos0 scale pos_dev pos_stride q_ld rope_cos rope_sin stream",
        dict(q=P, k=P, vt=P, out=P, kv_len=None, B=1, H=2, Lq=16, Skv=16, kv_stride=64, head_dim=128, causal=1, q_pos0=0,
             scale=0.125, pos_dev=None, pos_stride=0, q_ld=0, rope_cos=None, rope_sin=None, stream=None)),
    "gr_attention_paged": (
        "q k_pool vt_pool out kv_len B H Lq block_table table_ld head_dim q_pos0 scale pos_dev pos_stride q_ld rope_cos rope_sin stream",
        dict(q=P, k_pool=P, vt_pool=P, out=P, kv_len=None, B=1, H=2, Lq=16, block_table=P, table_ld=2, head_dim=128, q_pos0=0,
             scale=0.125, pos_dev=None, pos_stride=0, q_ld=0, rope_cos=None, rope_sin=None, stream=None)),
    "gr_decode_attention": (
        "q k vt out kv_len B H Smax kv_stride head_dim q_pos0 scale pos_dev pos_stride nsplit parts stream",
        dict(q=P, k=P, vt=P, out=P, kv_len=None, B=1, H=2, Smax=64, kv_stride=64, head_dim=128, q_pos0=0, scale=0.125,
             pos_dev=None, pos_stride=0, nsplit=1, parts=None, stream=None)),
    "gr_decode_attention_paged": (
        "q k_pool vt_pool out kv_len B H Smax block_table table_ld head_dim q_pos0 scale pos_dev pos_stride nsplit parts stream",
        dict(q=P, k_pool=P, vt_pool=P, out=P, kv_len=None, B=1, H=2, Smax=64, block_table=P, table_ld=1, head_dim=128, q_pos0=0,
             scale=0.125, pos_dev=None, pos_stride=0, nsplit=1, parts=None, stream=None)),
    "gr_qkv_split": (
        "qkv q k vt cosT sinT B H L head_dim pos0 kv_stride pos_dev pos_stride stream",
        dict(qkv=P, q=P, k=P, vt=P, cosT=None, sinT=None, B=1, H=2, L=16, head_dim=128, pos0=0, kv_stride=64, pos_dev=None,
             pos_stride=0, stream=None)),
    "gr_qkv_split_paged": (
        "qkv q k_pool vt_pool cosT sinT B H L head_dim pos0 block_table table_ld pos_dev pos_stride stream",
        dict(qkv=P, q=P, k_pool=P, vt_pool=P, cosT=None, sinT=None, B=1, H=2, L=1, head_dim=128, pos0=0, block_table=P,
             table_ld=2, pos_dev=None, pos_stride=0, stream=None)),
    "gr_kv_append_paged": (
        "qkv k_pool vt_pool cosT sinT B H L head_dim pos0 block_table table_ld pos_dev pos_stride stream",
        dict(qkv=P, k_pool=P, vt_pool=P, cosT=None, sinT=None, B=1, H=2, L=16, head_dim=128, pos0=0, block_table=P, table_ld=2,
             pos_dev=None, pos_stride=0, stream=None)),
}

NULLS = {  # required pointers
    "gr_attention_bf16": "q k vt out", "gr_attention_paged": "q k_pool vt_pool out block_table",
    "gr_decode_attention": "q k vt out", "gr_decode_attention_paged": "q k_pool vt_pool out block_table",
    "gr_qkv_split": "qkv k vt", "gr_qkv_split_paged": "qkv k_pool vt_pool block_table",
    "gr_kv_append_paged": "qkv k_pool vt_pool block_table",
}
SIZES = {  # must be positive
    "gr_attention_bf16": "B H Lq Skv", "gr_attention_paged": "B H Lq", "gr_decode_attention": "B H Smax",
    "gr_decode_attention_paged": "B H Smax", "gr_qkv_split": "B H L", "gr_qkv_split_paged": "B H L", "gr_kv_append_paged": "B H L",
}
Q_LD = [dict(q_ld=-8), dict(q_ld=260), dict(q_ld=248)]  # negative; not a multiple of 8; below H * hd = 256
ROPE = [dict(rope_cos=P), dict(rope_sin=P)]
ROPE_T = [dict(cosT=P), dict(sinT=P)]
HEAD_DIM = [dict(head_dim=96), dict(head_dim=0), dict(head_dim=256)]
NSPLIT = [dict(nsplit=0), dict(nsplit=17), dict(nsplit=2)]  # (2 without `parts`)
OTHER = {
    # kv_stride % 64; kv_stride < Skv (both ways round)
    "gr_attention_bf16": [dict(kv_stride=96), dict(kv_stride=0), dict(Skv=65)] + Q_LD + ROPE + HEAD_DIM,
    # table_ld outside 1 .. 8192 / KV_PAGE; host positions before / past the table
    "gr_attention_paged": [dict(table_ld=0), dict(table_ld=8192 // KV_PAGE + 1), dict(q_pos0=-1), dict(q_pos0=2 * KV_PAGE - 15)]
    + Q_LD + ROPE + HEAD_DIM,
    "gr_decode_attention": [dict(Smax=DEC_SMAX + 64, kv_stride=DEC_SMAX + 64), dict(kv_stride=96), dict(kv_stride=0), dict(q_pos0=64)]
    + NSPLIT + HEAD_DIM,
    "gr_decode_attention_paged": [dict(Smax=DEC_SMAX + 64, table_ld=DEC_SMAX // KV_PAGE + 1), dict(table_ld=0),
                                  dict(table_ld=DEC_SMAX // KV_PAGE + 1), dict(Smax=65), dict(q_pos0=-1), dict(q_pos0=64)]
    + NSPLIT + HEAD_DIM,
    "gr_qkv_split": ROPE_T + HEAD_DIM,
    "gr_qkv_split_paged": [dict(L=2), dict(table_ld=0), dict(table_ld=129), dict(pos0=-1), dict(pos0=2 * KV_PAGE)] + ROPE_T + HEAD_DIM,
    "gr_kv_append_paged": [dict(table_ld=0), dict(table_ld=129), dict(pos0=-1), dict(pos0=2 * KV_PAGE - 15)] + ROPE_T + HEAD_DIM,
}


def _violations(name):
    out = [{n: None} for n in NULLS[name].split()]
    out += [{n: v} for n in SIZES[name].split() for v in (0, -1)]
    return out + OTHER[name]


def _call(name, **override):
    names, valid = ENTRIES[name]
    args = dict(valid, **override)
    return getattr(_lib.load(), name)(*[args[n] for n in names.split()])


INVALID = [(name, v) for name in ENTRIES for v in _violations(name)]


@pytest.mark.parametrize("name,violation", INVALID, ids=[f"{n}-{'-'.join(f'{k}={v}' for k, v in d.items())}" for n, d in INVALID])
def test_one_bad_argument_is_rejected(name, violation):
    assert set(violation) <= set(ENTRIES[name][1])
    assert _call(name, **violation) == EINVAL


# what a valid call may differ in without becoming invalid: q left in the fused buffer; device-resident positions switch the
# host-position checks off; several key slices with a workspace
VALID = {
    "gr_decode_attention": [dict(), dict(pos_dev=P, q_pos0=64), dict(nsplit=16, parts=P), dict(head_dim=64)],
    "gr_decode_attention_paged": [dict(), dict(pos_dev=P, q_pos0=-1), dict(nsplit=16, parts=P), dict(head_dim=64)],
    "gr_qkv_split": [dict(), dict(q=None), dict(cosT=P, sinT=P), dict(head_dim=64)],
    "gr_qkv_split_paged": [dict(), dict(q=None), dict(pos_dev=P, pos0=-1), dict(head_dim=64)],
    "gr_kv_append_paged": [dict(), dict(pos_dev=P, pos0=-1), dict(cosT=P, sinT=P), dict(head_dim=64)],
}
VALID_CASES = [(name, v) for name in VALID for v in VALID[name]]


@pytest.mark.parametrize("name,change", VALID_CASES, ids=[f"{n}-{'-'.join(f'{k}={v}' for k, v in d.items()) or 'base'}" for n, d in VALID_CASES])
def test_valid_arguments_reach_the_launch(name, change):
    rc = _call(name, **change)
    assert rc != 0 and rc != EINVAL, rc
