"""-m gpu: the GEMM-composed attention (every head_dim but 64: csrc/attention.hip's generic branch of launch_attention and
csrc/attention_slp.hip's launch_attention_composed_len) on EVERY element, per utterance, against the fp64 reference of
tests/attn_ref.py restricted to each row's visible keys, within attn_ref.bound — the bound that
tests/test_attention_composed_bound.py shows to pass this path's arithmetic at <= 0.43 and to flag one key too few or too many,
the padded batch's causal offset and another head's V at >= 113.  The data (attn_ref.make_masked_case) put a dominant key on
both sides of every mask edge, so a row that passes saw exactly its keys.  Neither the bound nor the 1.0 is fitted.

Covered: the dense causal entry at head_dim 128 .. 1536 (Sq > Skv: rows that see nothing are exactly 0), the entry with lengths
(1 / 63 / 64 / 65 / full, q_len NULL, kl - ql != Skv - Sq, kl < ql; finite and NaN padding bitwise equal), the unmasked entries
at the shipped head (bf16 output, fp32 residual in place and out of place), the stack's strides (q | k | v and k | v windows of
one buffer, the output a window of a sentinel buffer), the forced GEMM tile structures, and the launchers' loop over chunks of
(batch, head) pairs, reached through the option "attn_generic_kib".

The chunked result against the unchunked one is printed, not asserted, bit for bit: launch_gemm (csrc/gemm.hip) sends a batched
launch (more than one pair) to the plain 128 x 128 kernel and a single pair to whatever its rule picks for the shape (the
deep-prefetch 128 x 128 kernel at K >= 256, others from "gemm_tile"), so a chunk of ONE pair may sum over k in another kernel than
a chunk of several.  Every chunking holds the bound on every element, which is what is asserted.

Measured on an MI355X (worst |err| / bound over all elements; inputs and kernels are deterministic, so these repeat):
  dense causal 0.384 (2 x 2 heads of 384, 130 x 130; 0.134 .. 0.384 over the shapes), with lengths 0.303 causal / 0.216 not
  (NaN padding: the same bits), unmasked at the shipped head 0.165 (bf16 output) / 0.196 (fp32 residual, either form), the stack's
  strides 0.347, forced gemm_tile 0.313 (the same under 0 / 128 / 256 / 192), the chunk loop 0.244 — and all nine chunked runs
  came out bit for bit the unchunked ones."""
import math

import pytest
import torch

from attn_ref import LOG2E, bound, make_masked_case, reference, visible_keys, worst_ratio
from ditto_tts_amd import hip
from gpu_util import asym, stream

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
KIB_DEFAULT = 2097152
SENT = 0x4F4F            # bf16 bits of a large finite value no result takes
WORST = {}


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    l = hip.lib()
    assert hip.get_option("attn_generic_kib") == KIB_DEFAULT and hip.get_option("gemm_tile") == 0
    yield l
    hip.set_option("attn_generic_kib", KIB_DEFAULT)
    hip.set_option("gemm_tile", 0)
    for name in sorted(WORST):
        print(f"composed attention, {name}: worst ratio {WORST[name]:.3f}")


def i32(v):
    return torch.tensor(list(v), dtype=torch.int32, device=DEV)


def _bits(t):
    return t.contiguous().view(torch.int16) if t.dtype == torch.bfloat16 else t.contiguous().view(torch.int32)


def fwd_bytes(Sq, Skv, dh):
    """scratch of ONE (batch, head) pair: csrc/attention.hip generic_fwd_bytes (fp32 scores, bf16 probabilities, V^T; 256-byte pieces)"""
    ld = (Skv + 63) // 64 * 64
    al = lambda x: (x + 255) & ~255
    return al(Sq * ld * 4) + al(Sq * ld * 2) + al(dh * ld * 2)


def chunks_of(B, H, room):
    """the launchers' chunk arithmetic: whole batches, or a divisor of H inside one batch"""
    c = min(room, B * H)
    if c >= H:
        c = c // H * H
    else:
        while H % c:
            c -= 1
    return [min(c, B * H - s) for s in range(0, B * H, c)]


def _ws(nbytes):
    return torch.empty(max(nbytes, 256), dtype=torch.uint8, device=DEV)


def run_causal(lib, q, ldq, k, ldk, v, ldv, out, ldo, B, H, Sq, Skv, dh, scale, lens=None, causal=True, short=0):
    """the dense causal entry (lens None) or the entry with lengths (lens = (q_len or None, kv_len)); pointers are addresses"""
    nb = lib.ditto_attention_causal_workspace_bytes(B, H, Sq, Skv, dh)
    assert nb > 0
    ws = _ws(nb)
    if lens is None:
        assert causal
        rc = lib.ditto_attention_causal_bf16(q, ldq, k, ldk, v, ldv, out, ldo, B, H, Sq, Skv, dh, scale, ws.data_ptr(),
                                             nb - short, stream())
    else:
        qld, kld = (None if n is None else i32(n) for n in lens)
        rc = lib.ditto_attention_causal_varlen_bf16(q, ldq, k, ldk, v, ldv, out, ldo, None if qld is None else qld.data_ptr(),
                                                    None if kld is None else kld.data_ptr(), B, H, Sq, Skv, dh, scale,
                                                    int(causal), ws.data_ptr(), nb - short, stream())
    torch.cuda.synchronize()
    return rc


def check_all(name, got, q, k, v, B, H, Sq, Skv, dh, scale, vis, stored_bf16=True, resid=None, key=None):
    """every element of got [B*Sq, H*dh] within the bound, per utterance; returns (and records) the worst ratio"""
    o, wabs, s1 = reference(q, k, v, B, H, Sq, Skv, dh, scale * LOG2E, vis=vis)
    want, e = bound(o, wabs, s1, Skv, dh, resid=resid)
    ratios = [worst_ratio(got[b * Sq:(b + 1) * Sq], want[b * Sq:(b + 1) * Sq], e[b * Sq:(b + 1) * Sq], stored_bf16) for b in range(B)]
    worst = max(ratios)
    print(f"{name}: worst |err| / bound = {worst:.3f}  (per utterance: {', '.join('%.3f' % r for r in ratios)})")
    if key:
        WORST[key] = max(WORST.get(key, 0.0), worst)
    assert worst <= 1.0, f"{name}: worst |err| / bound per utterance = {ratios}"
    if vis is not None:
        dark = (vis == 0).reshape(-1).to(got.device)
        assert bool((got[dark] == 0).all()), f"{name}: a row that sees no key is not exactly 0"
    return worst


def check_sharp(name, got, q, k, v, B, H, Sq, Skv, dh, scale, vis, q_len=None):
    """the control: the SAME output held against the reference of a mask with one key fewer, and with one key more, is far outside
    the bound — the case can tell such a kernel from a right one (a condition on the data, as in test_attention_composed_bound.py)"""
    valid = visible_keys(B, Sq, Skv, q_len) > 0
    for tag, n in (("fewer", (vis - 1).clamp_min(0)), ("more", torch.where(valid, (vis + 1).clamp_max(Skv), vis))):
        if torch.equal(n, vis):
            continue
        o, wabs, s1 = reference(q, k, v, B, H, Sq, Skv, dh, scale * LOG2E, vis=n)
        want, e = bound(o, wabs, s1, Skv, dh)
        r = worst_ratio(got, want, e, True)
        assert r > 2.0, f"{name}: one key {tag} would pass ({r:.3f}): the case is not sharp"


# ------------------------------------------------------------------ the dense causal entry
@pytest.mark.parametrize("B,H,Sq,Skv,dh", [(1, 1, 1, 1, 1536), (2, 4, 40, 40, 128), (1, 2, 97, 97, 192), (2, 2, 130, 130, 384),
                                           (2, 1, 33, 70, 768), (1, 3, 64, 65, 128), (1, 2, 257, 63, 192), (2, 2, 70, 33, 384)])
def test_dense_causal(lib, B, H, Sq, Skv, dh):
    """the mask aligned to the END of the keys; Sq > Skv: the first Sq - Skv rows see no key and are exactly 0"""
    D = H * dh
    q, k, v, scale = make_masked_case(B, H, Sq, Skv, dh, 310, causal=True, device=DEV)
    out = torch.full((B * Sq, D), 777.0, dtype=torch.bfloat16, device=DEV)
    hip.check(run_causal(lib, q.data_ptr(), D, k.data_ptr(), D, v.data_ptr(), D, out.data_ptr(), D, B, H, Sq, Skv, dh, scale))
    vis = visible_keys(B, Sq, Skv, causal=True)
    assert Sq <= Skv or int((vis == 0).sum()) == B * (Sq - Skv)
    check_all(f"dense causal B{B} H{H} {Sq}x{Skv} dh{dh}", out, q, k, v, B, H, Sq, Skv, dh, scale, vis, key="dense causal")
    check_sharp(f"dense causal B{B} H{H} {Sq}x{Skv} dh{dh}", out, q, k, v, B, H, Sq, Skv, dh, scale, vis)


# ------------------------------------------------------------------ the entry with lengths
LEN_CASES = [
    (3, 2, 130, 130, 128, True, [1, 63, 130], [1, 63, 130]),
    (2, 2, 130, 130, 384, True, [64, 65], [64, 65]),
    (2, 2, 33, 70, 192, True, [33, 5], [70, 64]),            # kl - ql = 37, 59; Skv - Sq = 37
    (2, 1, 70, 70, 768, True, [1, 65], [1, 64]),             # kl < ql: row 0 of utterance 1 sees no key
    (2, 1, 40, 80, 1536, True, None, [63, 80]),              # q_len NULL = Sq
    (3, 2, 33, 70, 128, False, [33, 5, 20], [70, 1, 33]),
    (3, 1, 33, 70, 768, False, None, [64, 65, 70]),
    (2, 2, 65, 130, 192, False, [1, 64], [63, 65]),
]


@pytest.mark.parametrize("B,H,Sq,Skv,dh,causal,q_len,kv_len", LEN_CASES)
def test_composed_with_lengths(lib, B, H, Sq, Skv, dh, causal, q_len, kv_len):
    """finite padding (K row kl is an aligned key: seeing it moves a row by O(|v|)), then NaN in every padded q / k / v row: valid
    rows bitwise equal, rows at or past q_len exactly 0, every element within the bound of the utterance's OWN mask"""
    D = H * dh
    q0, k0, v0, scale = make_masked_case(B, H, Sq, Skv, dh, 320, q_len, kv_len, causal, device=DEV)
    ql = q_len if q_len is not None else [Sq] * B
    vis = visible_keys(B, Sq, Skv, q_len, kv_len, causal)
    outs = []
    for fill in (None, NAN):
        q, k, v = q0.clone(), k0.clone(), v0.clone()
        if fill is not None:
            for b in range(B):
                q[b * Sq + ql[b]:(b + 1) * Sq] = fill
                k[b * Skv + kv_len[b]:(b + 1) * Skv] = fill
                v[b * Skv + kv_len[b]:(b + 1) * Skv] = fill
        out = torch.full((B * Sq, D), 777.0, dtype=torch.bfloat16, device=DEV)
        hip.check(run_causal(lib, q.data_ptr(), D, k.data_ptr(), D, v.data_ptr(), D, out.data_ptr(), D, B, H, Sq, Skv, dh, scale,
                             lens=(q_len, kv_len), causal=causal))
        tag = "causal" if causal else "full"
        check_all(f"lengths {tag} B{B} H{H} {Sq}x{Skv} dh{dh} q{q_len} kv{kv_len} padding {'NaN' if fill else 'finite'}",
                  out, q, k, v, B, H, Sq, Skv, dh, scale, vis, key=f"with lengths, {tag}")
        if fill is None:
            check_sharp(f"lengths {tag} B{B} H{H} {Sq}x{Skv} dh{dh}", out, q, k, v, B, H, Sq, Skv, dh, scale, vis, q_len)
        outs.append(out)
    for b in range(B):
        assert bool((outs[0][b * Sq + ql[b]:(b + 1) * Sq] == 0).all()) and bool((outs[1][b * Sq + ql[b]:(b + 1) * Sq] == 0).all())
        valid = slice(b * Sq, b * Sq + ql[b])
        assert torch.equal(_bits(outs[0][valid]), _bits(outs[1][valid])), f"utterance {b}: NaN padding changed a valid row"


# ------------------------------------------------------------------ dense, unmasked, at the shipped head
@pytest.mark.parametrize("form", ["bf16_out", "resid_inplace", "resid_outofplace"])
@pytest.mark.parametrize("B,H,Sq,Skv,dh", [(2, 1, 130, 200, 768), (1, 2, 65, 64, 384)])
def test_dense_unmasked_at_the_shipped_head(lib, B, H, Sq, Skv, dh, form):
    D, ldr = H * dh, H * dh + 8
    q, k, v, scale = make_masked_case(B, H, Sq, Skv, dh, 330, device=DEV)
    nb = lib.ditto_attention_workspace_bytes(B, H, Sq, Skv, dh)
    assert nb > 0
    ws = _ws(nb)
    name = f"unmasked {form} B{B} H{H} {Sq}x{Skv} dh{dh}"
    if form == "bf16_out":
        out = torch.full((B * Sq, D), 777.0, dtype=torch.bfloat16, device=DEV)
        hip.check(lib.ditto_attention_bf16(q.data_ptr(), D, k.data_ptr(), D, v.data_ptr(), D, out.data_ptr(), D, B, H, Sq, Skv, dh,
                                           scale, ws.data_ptr(), nb, stream()))
        torch.cuda.synchronize()
        check_all(name, out, q, k, v, B, H, Sq, Skv, dh, scale, None, key="unmasked, bf16 output")
        return
    resid = asym((B * Sq, D), 333).to(DEV)
    rin = torch.full((B * Sq + 2, ldr), -12345.5, dtype=torch.float32, device=DEV)     # two guard rows, eight guard columns
    rin[:B * Sq, :D] = resid
    rin0 = rin.clone()
    rout = rin if form == "resid_inplace" else torch.full_like(rin, -12345.5)
    rout0 = rout.clone()
    hip.check(lib.ditto_attention_resid_bf16(q.data_ptr(), D, k.data_ptr(), D, v.data_ptr(), D,
                                             None if form == "resid_inplace" else rin.data_ptr(), rout.data_ptr(), ldr, 0, B, H,
                                             Sq, Skv, dh, scale, ws.data_ptr(), nb, stream()))
    torch.cuda.synchronize()
    check_all(name, rout[:B * Sq, :D], q, k, v, B, H, Sq, Skv, dh, scale, None, stored_bf16=False, resid=resid,
              key="unmasked, fp32 residual")
    assert torch.equal(_bits(rout[:, D:]), _bits(rout0[:, D:])) and torch.equal(_bits(rout[B * Sq:]), _bits(rout0[B * Sq:]))
    if form != "resid_inplace":
        assert torch.equal(_bits(rin), _bits(rin0)), "the input stream was written"


# ------------------------------------------------------------------ the stack's strides
def _window(rows, D):
    """a [rows, D] window at row stride D + 64 of a sentinel-filled bf16 buffer, three guard rows before and after"""
    ldo, guard = D + 64, 3
    buf = torch.full(((rows + 2 * guard) * ldo,), SENT, dtype=torch.int16, device=DEV).view(torch.bfloat16)
    win = buf[guard * ldo:(guard + rows) * ldo].view(rows, ldo)
    inside = torch.zeros(rows + 2 * guard, ldo, dtype=torch.bool, device=DEV)
    inside[guard:guard + rows, :D] = True
    return buf, win, ldo, inside.view(-1)


@pytest.mark.parametrize("layout", ["qkv_dense", "qkv_lengths", "kv_lengths"])
def test_the_stacks_strides(lib, layout):
    """q | k | v windows of one [rows, 3 D] buffer (self-attention: ldq = ldk = ldv = 3 D), q of its own and k | v windows of a
    [rows, 2 D] buffer (cross-attention); the output a window of a sentinel buffer whose sentinels come back bit for bit"""
    if layout == "kv_lengths":
        B, H, Sq, Skv, dh, causal, q_len, kv_len = 2, 2, 33, 70, 192, False, None, [70, 33]
    else:
        B, H, Sq, Skv, dh, causal = 2, 2, 97, 97, 128, True
        q_len, kv_len = ([97, 40], [97, 40]) if layout == "qkv_lengths" else (None, None)
    D = H * dh
    qc, kc, vc, scale = make_masked_case(B, H, Sq, Skv, dh, 340, q_len, kv_len, causal, device=DEV)
    if layout == "kv_lengths":
        src = torch.full((B * Skv, 2 * D), 3.0, dtype=torch.bfloat16, device=DEV)
        src[:, :D], src[:, D:] = kc, vc
        q, k, v, ldq, ldk = qc, src[:, :D], src[:, D:], D, 2 * D
        ptrs = (q.data_ptr(), src.data_ptr(), src.data_ptr() + 2 * D)
    else:
        src = torch.full((B * Sq, 3 * D), 3.0, dtype=torch.bfloat16, device=DEV)
        src[:, :D], src[:, D:2 * D], src[:, 2 * D:] = qc, kc, vc
        q, k, v, ldq, ldk = src[:, :D], src[:, D:2 * D], src[:, 2 * D:], 3 * D, 3 * D
        ptrs = (src.data_ptr(), src.data_ptr() + 2 * D, src.data_ptr() + 4 * D)
    buf, win, ldo, inside = _window(B * Sq, D)
    before = buf.clone()
    hip.check(run_causal(lib, ptrs[0], ldq, ptrs[1], ldk, ptrs[2], ldk, win.data_ptr(), ldo, B, H, Sq, Skv, dh, scale,
                         lens=None if layout == "qkv_dense" else (q_len, kv_len), causal=causal))
    assert torch.equal(_bits(buf)[~inside], _bits(before)[~inside]), "written outside the output window"
    vis = visible_keys(B, Sq, Skv, q_len, kv_len, causal)
    check_all(f"strides {layout}", win[:, :D], q, k, v, B, H, Sq, Skv, dh, scale, vis, key="the stack's strides")


# ------------------------------------------------------------------ GEMM tile structures
@pytest.mark.parametrize("tile", [0, 128, 256, 192])
@pytest.mark.parametrize("B,H,Sq,Skv,dh,q_len,kv_len", [(1, 1, 130, 130, 384, None, None), (1, 1, 97, 140, 768, [65], [100]),
                                                        (2, 2, 40, 40, 128, [40, 7], [40, 33])])
def test_under_each_gemm_tile_structure(lib, tile, B, H, Sq, Skv, dh, q_len, kv_len):
    """"gemm_tile" reaches this path's two GEMMs where a launch holds ONE (batch, head) pair (batched launches always take the
    128 x 128 kernel): the first two shapes; the third shows that a batched launch is indifferent to it"""
    D = H * dh
    q, k, v, scale = make_masked_case(B, H, Sq, Skv, dh, 350, q_len, kv_len, True, device=DEV)
    out = torch.full((B * Sq, D), 777.0, dtype=torch.bfloat16, device=DEV)
    try:
        hip.set_option("gemm_tile", tile)
        hip.check(run_causal(lib, q.data_ptr(), D, k.data_ptr(), D, v.data_ptr(), D, out.data_ptr(), D, B, H, Sq, Skv, dh, scale,
                             lens=None if kv_len is None else (q_len, kv_len)))
    finally:
        hip.set_option("gemm_tile", 0)
    check_all(f"gemm_tile {tile} B{B} H{H} {Sq}x{Skv} dh{dh} q{q_len} kv{kv_len}", out, q, k, v, B, H, Sq, Skv, dh, scale,
              visible_keys(B, Sq, Skv, q_len, kv_len, True), key="forced gemm_tile")


# ------------------------------------------------------------------ the chunk loop
def _set_room(lib, B, H, Sq, Skv, dh, room):
    """the budget under which the size query admits `room` pairs; returns the bytes of one pair"""
    one = fwd_bytes(Sq, Skv, dh)
    assert one >= 1024
    hip.set_option("attn_generic_kib", (room * one + 1023) // 1024)
    assert lib.ditto_attention_causal_workspace_bytes(B, H, Sq, Skv, dh) == room * one, "the size query does not follow the option"
    assert lib.ditto_attention_workspace_bytes(B, H, Sq, Skv, dh) == room * one
    return one


@pytest.mark.parametrize("entry", ["dense_causal", "lengths", "resid"])
@pytest.mark.parametrize("B,H,room,expect", [(3, 2, 5, [4, 2]), (2, 4, 3, [2, 2, 2, 2]), (2, 3, 2, [1] * 6)])
def test_chunk_loop(lib, entry, B, H, room, expect):
    """a budget smaller than B H pairs: whole batches (4 then 2), a divisor of H inside one batch (2), one pair at a time.  Distinct data
    per batch and head, so a wrong b0 / h0 offset or a wrong stride in a later chunk lands on another pair's rows."""
    assert chunks_of(B, H, room) == expect and len(expect) > 1
    Sq, Skv, dh = 40, 70, 128
    D = H * dh
    causal = entry != "resid"
    q_len, kv_len = ([40, 7, 33][:B], [70, 33, 64][:B]) if entry == "lengths" else (None, None)
    q, k, v, scale = make_masked_case(B, H, Sq, Skv, dh, 360, q_len, kv_len, causal, device=DEV)
    vis = visible_keys(B, Sq, Skv, q_len, kv_len, True) if causal else None
    resid = asym((B * Sq, D), 363).to(DEV)

    def run():
        if entry == "resid":
            nb = lib.ditto_attention_workspace_bytes(B, H, Sq, Skv, dh)
            ws, r = _ws(nb), resid.clone()
            hip.check(lib.ditto_attention_resid_bf16(q.data_ptr(), D, k.data_ptr(), D, v.data_ptr(), D, None, r.data_ptr(), D, 0, B, H,
                                                     Sq, Skv, dh, scale, ws.data_ptr(), nb, stream()))
            torch.cuda.synchronize()
            return r
        out = torch.full((B * Sq, D), 777.0, dtype=torch.bfloat16, device=DEV)
        hip.check(run_causal(lib, q.data_ptr(), D, k.data_ptr(), D, v.data_ptr(), D, out.data_ptr(), D, B, H, Sq, Skv, dh, scale,
                             lens=None if entry == "dense_causal" else (q_len, kv_len)))
        return out

    whole = run()
    try:
        one = _set_room(lib, B, H, Sq, Skv, dh, room)
        chunked = run()
        # one byte short of what the query asks for is refused, on every entry
        out = torch.empty(B * Sq, D, dtype=torch.bfloat16, device=DEV)
        assert run_causal(lib, q.data_ptr(), D, k.data_ptr(), D, v.data_ptr(), D, out.data_ptr(), D, B, H, Sq, Skv, dh, scale,
                          lens=None if entry != "lengths" else (q_len, kv_len), short=1) == hip.ERR_SIZE
        ws = _ws(room * one)
        r = resid.clone()
        assert lib.ditto_attention_resid_bf16(q.data_ptr(), D, k.data_ptr(), D, v.data_ptr(), D, None, r.data_ptr(), D, 0, B, H, Sq,
                                              Skv, dh, scale, ws.data_ptr(), room * one - 1, stream()) == hip.ERR_SIZE
        torch.cuda.synchronize()
        assert torch.equal(r, resid), "a refused call wrote the stream"
    finally:
        hip.set_option("attn_generic_kib", KIB_DEFAULT)
    assert lib.ditto_attention_causal_workspace_bytes(B, H, Sq, Skv, dh) == B * H * fwd_bytes(Sq, Skv, dh)
    name = f"chunks {expect} {entry} B{B} H{H}"
    for tag, got in (("unchunked", whole), ("chunked", chunked)):
        check_all(f"{name} {tag}", got, q, k, v, B, H, Sq, Skv, dh, scale, vis, stored_bf16=entry != "resid",
                  resid=resid if entry == "resid" else None, key="chunk loop" if tag == "chunked" else None)
    print(f"{name}: bitwise the unchunked result: {torch.equal(_bits(whole), _bits(chunked))}")


def test_the_budget_option_refuses_zero(lib):
    assert lib.ditto_set_option(b"attn_generic_kib", 0) == hip.ERR_ARG
    assert lib.ditto_set_option(b"attn_generic_kib", -5) == hip.ERR_ARG
    assert hip.get_option("attn_generic_kib") == KIB_DEFAULT
    # the floor of one pair: a budget below one pair's scratch still asks for (and runs with) one pair
    try:
        hip.set_option("attn_generic_kib", 1)
        assert lib.ditto_attention_causal_workspace_bytes(2, 2, 40, 70, 128) == fwd_bytes(40, 70, 128)
    finally:
        hip.set_option("attn_generic_kib", KIB_DEFAULT)
