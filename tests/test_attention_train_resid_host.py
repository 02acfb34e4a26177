"""ditto_attention_train_resid_bf16 on a GPU-less host: the entry refuses, before any HIP call, what its launch cannot serve — in the
order DITTO_ERR_SHAPE, DITTO_ERR_ARG, DITTO_ERR_SIZE — in the manner of test_train_rows_host.py: one valid argument set per layout
(dense, packed) with fake, aligned, non-null addresses, then one argument at a time.  Only refused calls are made here: the valid calls
are made by test_gpu_attention_train_fwd_elementwise.py on a GPU."""
import pytest

from ditto_tts_amd import hip

ENTRY = "ditto_attention_train_resid_bf16"
POINTERS = {"q": 16, "k": 16, "v": 16, "resid_in": 16, "resid_out": 16, "out": 8, "lse_out": 4, "cu_q": 4, "cu_kv": 4}   # name: alignment
OPTIONAL = {"resid_in", "out"}


def args(packed, bf16_stream=False):
    """a valid call: B = 2, H = 3; dense 100 x 72 per utterance, packed 140 / 90 rows in all; the model's strides"""
    B, H, d = 2, 3, 192
    rq, rk = (140, 90) if packed else (B * 100, B * 72)
    ld = dict(ldq=3 * d, ldk=3 * d, ldv=3 * d, ldr=d + 8, ldo=d)
    esz = 2 if bf16_stream else 4
    size = dict(q=((rq - 1) * ld["ldq"] + d) * 2, k=((rk - 1) * ld["ldk"] + d) * 2, v=((rk - 1) * ld["ldv"] + d) * 2,
                resid_in=((rq - 1) * ld["ldr"] + d) * esz, resid_out=((rq - 1) * ld["ldr"] + d) * esz, out=((rq - 1) * ld["ldo"] + d) * 2,
                lse_out=rq * H * 4, cu_q=(B + 1) * 4, cu_kv=(B + 1) * 4)
    kw, addr = dict(ld), 1 << 20
    for n in POINTERS:
        dense_null = n.startswith("cu_") and not packed
        kw[n], kw[n + "_bytes"] = (None, 0) if dense_null else (addr, size[n])
        addr += (size[n] + 8191) // 4096 * 4096
    kw.update(resid_bf16=int(bf16_stream), B=B, H=H, Sq=rq if packed else 100, Skv=rk if packed else 72, max_q=80 if packed else 100,
              max_kv=50 if packed else 72, dh=64, scale=0.125, dropout_p=0.1, seed=7, layer=3, stream=None)
    return kw


def refused(kw, code, flags=3):
    try:
        hip.set_option("attn_flags", flags)
        rc = hip.call(ENTRY, **kw)
    finally:
        hip.set_option("attn_flags", 3)
    msg = hip.lib().ditto_last_error().decode()
    assert rc == code and rc != hip.OK, (rc, code, msg)
    assert ENTRY in msg, msg
    return msg


@pytest.mark.parametrize("packed", [False, True], ids=["dense", "packed"])
@pytest.mark.parametrize("bf16_stream", [False, True], ids=["fp32", "bf16"])
def test_pointers_and_sizes_are_refused_one_at_a_time(packed, bf16_stream):
    kw = args(packed, bf16_stream)
    for n, align in POINTERS.items():
        if kw[n] is None:
            continue
        if n not in OPTIONAL:   # (one of cu_q / cu_kv alone: "given together")
            msg = refused(dict(kw, **{n: None}), hip.ERR_ARG)
            assert n in msg or "cu_q and cu_kv" in msg
        a = 8 if bf16_stream and n.startswith("resid") else align
        assert n in refused(dict(kw, **{n: kw[n] + a // 2}), hip.ERR_ARG)
        assert n in refused(dict(kw, **{n + "_bytes": kw[n + "_bytes"] - 1}), hip.ERR_SIZE)
        assert n in refused(dict(kw, **{n + "_bytes": 0}), hip.ERR_SIZE)


@pytest.mark.parametrize("packed", [False, True], ids=["dense", "packed"])
def test_shape_and_argument_rules_are_refused_one_at_a_time(packed):
    kw = args(packed)
    for over in (dict(dh=128), dict(dh=32), dict(B=0), dict(H=0), dict(Sq=0), dict(Skv=-1), dict(max_q=0), dict(layer=-1), dict(B=65536),
                 dict(ldq=kw["ldq"] + 4), dict(ldk=kw["ldk"] + 2), dict(ldv=kw["ldv"] + 1), dict(ldr=kw["ldr"] + 4), dict(ldo=kw["ldo"] + 4),
                 dict(ldq=184), dict(ldr=184), dict(ldo=184), dict(max_q=kw["Sq"] + 1), dict(max_kv=kw["Skv"] + 1)):
        refused(dict(kw, **over), hip.ERR_SHAPE)
    if packed:
        refused(dict(kw, B=91), hip.ERR_SHAPE)          # more utterances than key rows
    else:
        refused(dict(kw, max_q=kw["Sq"] - 1), hip.ERR_SHAPE)   # dense: max_q is Sq
    for over in (dict(resid_bf16=2), dict(dropout_p=1.0), dict(dropout_p=-0.1), dict(dropout_p=float("nan")), dict(scale=float("inf")),
                 dict(cu_q=1 << 12, cu_q_bytes=64) if not packed else dict(cu_kv=None)):
        refused(dict(kw, **over), hip.ERR_ARG)
    # the order: a shape error wins over an argument error, an argument error over a size error
    refused(dict(kw, dh=128, lse_out=None, q_bytes=0), hip.ERR_SHAPE)
    refused(dict(kw, lse_out=None, q_bytes=0), hip.ERR_ARG)


def test_a_grown_shape_is_a_size_error_not_a_launch():
    """one more utterance, row or head than the buffers hold"""
    for packed, over in ((False, dict(B=3)), (False, dict(Sq=101, max_q=101)), (False, dict(Skv=73, max_kv=73)), (True, dict(Sq=141)),
                         (True, dict(Skv=91)), (True, dict(B=3))):
        refused(dict(args(packed), **over), hip.ERR_SIZE)


def test_older_kernel_route_has_no_bf16_stream_no_o_beside_and_no_packed_batch():
    """attn_flags 8192 (attn64_kernel<.., TRAIN>): what launch_attention refuses, or would silently not write, is refused here"""
    for kw in (args(False, bf16_stream=True), args(False), args(True)):
        assert "8192" in refused(kw, hip.ERR_ARG, flags=8192)
    kw = args(False)
    assert hip.get_option("attn_flags") == 3
    # without `out` the dense fp32 stream is served by the older kernel: nothing left to refuse but a size
    assert "resid_out" in refused(dict(kw, out=None, out_bytes=0, resid_out_bytes=0), hip.ERR_SIZE, flags=8192)
