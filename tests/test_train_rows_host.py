"""The entries of include/ditto_train_rows.h on a GPU-less host: each refuses, before any HIP call, what its kernel cannot serve.  For
every entry one valid argument set of the case tables (train_rows_ref.host_arg_sets) with fake, aligned, non-null addresses; then, one
argument at a time: a null pointer, a misaligned pointer, each buffer one byte too small, each shape rule broken.  Only refused calls
are made here: the valid call of every set is made by test_gpu_train_rows.py on a GPU."""
import pytest

import train_rows_ref as T
from ditto_tts_amd import hip

SETS = T.host_arg_sets()


def fake_addresses():
    nxt = [1 << 20]

    def address(b):
        a = nxt[0]
        nxt[0] += (b.nbytes + 4095) // 4096 * 4096 + 4096
        return a                                              # 4096-byte aligned: every alignment an entry asks for
    return address


def refused(name, kw, code):
    rc = hip.call(name, **kw)
    msg = hip.lib().ditto_last_error().decode()
    assert rc == code and rc != hip.OK, (name, rc, code, msg)
    assert name in msg, msg
    return msg


def test_every_entry_has_an_argument_set():
    entries = {e for e, _, _ in SETS.values()}
    assert entries == {n for n in hip.TRAIN_ROWS_PROTOTYPES if not n.endswith("_scratch_bytes")}
    for label, (name, args, _) in SETS.items():
        kw = T.materialise(args, fake_addresses())
        assert set(kw) == {p for p, _ in hip.TRAIN_ROWS_PROTOTYPES[name][1]}, label


@pytest.mark.parametrize("label", list(SETS))
def test_pointers_and_sizes_are_refused_one_at_a_time(label):
    name, args, _ = SETS[label]
    kw = T.materialise(args, fake_addresses())
    tried = 0
    for k, b in args.items():
        if not isinstance(b, T.Buf):
            continue
        if not b.optional:
            assert k in refused(name, dict(kw, **{k: None}), hip.ERR_ARG)
            tried += 1
        elif label == "gated":                                # colsum and scratch come together
            refused(name, dict(kw, **{k: None}), hip.ERR_ARG)
        if b.align > 1:
            assert k in refused(name, dict(kw, **{k: kw[k] + b.align // 2}), hip.ERR_ARG)
        assert k in refused(name, dict(kw, **{k + "_bytes": b.nbytes - 1}), hip.ERR_SIZE)
        assert k in refused(name, dict(kw, **{k + "_bytes": 0}), hip.ERR_SIZE)
        tried += 3
    assert tried >= 6


@pytest.mark.parametrize("label", list(SETS))
def test_shape_rules_are_refused_one_at_a_time(label):
    name, args, broken = SETS[label]
    address = fake_addresses()
    kw = T.materialise(args, address)
    assert broken
    for over, code in broken:
        refused(name, dict(kw, **T.materialise(over, address)), code)


def test_a_grown_shape_is_a_size_error_not_a_launch():
    """one more row, one more column, one more utterance than the buffers hold"""
    address = fake_addresses()
    for label, over in (("ln_stream", dict(rows=38)), ("adaln_packed", dict(S=59)), ("adaln_packed", dict(B=4)), ("gated", dict(M=34)),
                        ("colsum", dict(M=8)), ("reduce_partials", dict(chunks=18)), ("reduce_partials", dict(n=34)), ("transpose", dict(rows=66)),
                        ("transpose", dict(nz_o=3)), ("softmax_drop_rows", dict(nrows=16)), ("softmax_rows", dict(Skv=66)),
                        ("small_linear_fwd", dict(O=6)), ("small_linear_bwd_w", dict(I=66)), ("small_linear_bwd_x", dict(B=4)),
                        ("scatter", dict(V=6)), ("pack_bf16_t", dict(cols=41)), ("unpack_rows", dict(row_off=17)), ("unpack_vec", dict(rows=97))):
        name, args, _ = SETS[label]
        refused(name, dict(T.materialise(args, address), **over), hip.ERR_SIZE)


def test_call_names_the_new_header():
    with pytest.raises(TypeError, match="ditto_bwd_nothing: include/ditto_train_rows.h declares no such entry"):
        hip.call("ditto_bwd_nothing")
    with pytest.raises(TypeError, match="ditto_bwd_unpack_vec: missing src_bytes"):
        kw = T.materialise(SETS["unpack_vec"][1], fake_addresses())
        del kw["src_bytes"]
        hip.call("ditto_bwd_unpack_vec", **kw)
