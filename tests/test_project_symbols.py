"""include/ditto_project.h (no GPU), a table of its own beside ditto_hip.h's: declared = exported = bound; ditto_hip.h's table is what
it was (143 functions, ABI 10); the struct and the scratch arithmetic; the entries' argument checks, which run before any launch."""
import ctypes as C
import os
import re

from ditto_tts_amd import hip
from test_cabi_symbols import ROOT, declared_functions

NEW = ("ditto_guidance_project_bytes", "ditto_guidance_project_packed", "ditto_guided_update_packed_project",
       "ditto_multistep_update_packed_project", "ditto_guided_step_packed_project_opts",
       "ditto_guided_step_packed_multistep_project_opts")
P = 4096   # a non-NULL, 256-byte aligned pointer value: every call below fails its argument checks before anything touches it


def test_declared_exported_and_bound():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ditto_project.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(ditto_[a-z0-9_]+)\s*\(", txt)))
    assert names == sorted(NEW)
    assert sorted(hip.PROJECT_PROTOTYPES) == sorted(hip.PROJECT_SYMBOLS) == names
    lib = hip.lib()
    for n in names:
        assert hasattr(lib, n), f"{n} declared in ditto_project.h but not exported by libditto_hip.so"
        fn = getattr(lib, n)
        assert fn.argtypes == hip.PROJECT_SYMBOLS[n][1] and fn.restype == hip.PROJECT_SYMBOLS[n][0]
        assert [p for p, _ in hip.PROJECT_PROTOTYPES[n][1]] == list(hip._ORDER[n])
    assert hip.PROJECT_SYMBOLS["ditto_guidance_project_bytes"][0] is C.c_size_t


def test_ditto_hip_h_table_is_unchanged():
    names = declared_functions()
    assert len(names) == 143 and sorted(hip.SYMBOLS) == names
    assert not set(NEW) & set(names)
    for other in (hip.OPTIM_SYMBOLS, hip.TRAIN_ROWS_SYMBOLS, hip.TEXT_GRAD_SYMBOLS, hip.REFRESH_SYMBOLS):
        assert not set(NEW) & set(other)
    assert hip.lib().ditto_abi_version() == 10


def test_struct_and_scratch_arithmetic():
    assert C.sizeof(hip.ProjectCoef) == 32
    assert [f for f, _ in hip.ProjectCoef._fields_] == ["kx", "ke", "w", "eta", "r", "beta", "use_prev", "reserved"]
    lib = hip.lib()
    al = lambda n: (n + 255) // 256 * 256
    for B, max_N, d in ((1, 1, 64), (3, 96, 256), (32, 2000, 768), (7, 64, 256), (7, 65, 256), (4, 22, 768), (300, 17, 1024)):
        chunks = -(-(max_N * d // 4) // hip.RESCALE_CHUNK_QUADS)
        assert lib.ditto_guidance_project_bytes(B, max_N, d) == al(16 * B) + al(B * chunks * 32), (B, max_N, d)
        assert hip.project_scratch_layout(B) == al(16 * B)
    for bad in ((0, 5, 64), (2, 0, 64), (2, 5, 0), (2, 5, 96)):
        assert lib.ditto_guidance_project_bytes(*bad) == 0
        assert b"ditto_guidance_project_bytes" in lib.ditto_last_error()


def _refused(name, base, cases):
    lib = hip.lib()
    for kw, code, word in cases:
        a = dict(base)
        a.update(kw)
        assert hip.call(name, **a) == code, (name, kw)
        assert word in lib.ditto_last_error(), (name, kw, lib.ditto_last_error())


def test_entry_argument_checks_before_any_launch():
    need = hip.lib().ditto_guidance_project_bytes(3, 9, 256)
    rows = dict(cu=P, prompt_len=None, suffix_len=None, B=3, S=15, max_N=9, d=256, stream=None)
    shape_cases = [(dict(d=96), hip.ERR_SHAPE, b"% 64"), (dict(max_N=16), hip.ERR_SHAPE, b"max_N <= S"), (dict(B=0), hip.ERR_SHAPE, b"positive"),
                   (dict(B=16), hip.ERR_SHAPE, b"at least one row"), (dict(x2=None), hip.ERR_ARG, b"null"), (dict(eps2=None), hip.ERR_ARG, b"null"),
                   (dict(dir=None), hip.ERR_ARG, b"null"), (dict(cu=None), hip.ERR_ARG, b"null"), (dict(x2=P + 4), hip.ERR_ARG, b"16-byte"),
                   (dict(dir=P + 8), hip.ERR_ARG, b"16-byte")]
    _refused("ditto_guidance_project_packed", dict(x2=P, eps2=P, dir=P, proj=P, scratch=P, scratch_bytes=need, **rows), shape_cases + [
        (dict(proj=None), hip.ERR_ARG, b"null"), (dict(scratch=None), hip.ERR_ARG, b"null"), (dict(proj=P + 8), hip.ERR_ARG, b"16-byte"),
        (dict(scratch=P + 16), hip.ERR_ARG, b"256-byte"), (dict(scratch_bytes=need - 1), hip.ERR_SIZE, b"ditto_guidance_project_bytes")])
    ddim = dict(x2=P, eps2=P, dir=P, pcoef=P, noise=None, seeds=None, step=0, tags=None, a=P, ce=P, cz=P, **rows)
    _refused("ditto_guided_update_packed_project", ddim, shape_cases + [
        (dict(pcoef=None), hip.ERR_ARG, b"pcoef"), (dict(pcoef=P + 4), hip.ERR_ARG, b"pcoef"), (dict(noise=P, seeds=P), hip.ERR_ARG, b"exclusive"),
        (dict(noise=P + 4), hip.ERR_ARG, b"16-byte"), (dict(a=None), hip.ERR_ARG, b"null a"), (dict(ce=None), hip.ERR_ARG, b"null a"),
        (dict(seeds=P, cz=None), hip.ERR_ARG, b"null a")])
    ms = dict(x2=P, eps2=P, q=P, dir=P, pcoef=P, step=None, coefs=P, **rows)
    _refused("ditto_multistep_update_packed_project", ms, shape_cases + [
        (dict(pcoef=None), hip.ERR_ARG, b"pcoef"), (dict(q=None), hip.ERR_ARG, b"q "), (dict(q=P + 4), hip.ERR_ARG, b"q "),
        (dict(coefs=None), hip.ERR_ARG, b"exactly one"), (dict(step=hip.MultistepCoef()), hip.ERR_ARG, b"exactly one"),
        (dict(coefs=P + 8), hip.ERR_ARG, b"16-byte")])
    # the step entries refuse a null model before anything else
    common = dict(m=None, x2=P, cond=P, t=P, cu_speech=P, cu_text=P, prompt_len=None, suffix_len=None, dir=P, proj=P, B=3, S=15, max_N=9, S_T=9,
                max_T=3, rope_cos=P, rope_sin=P, workspace=P, workspace_bytes=1 << 20, scratch=P, scratch_bytes=need, stream=None, opts=None)
    assert hip.call("ditto_guided_step_packed_project_opts", noise=None, seeds=None, step=0, tags=None, a=P, ce=P, cz=P, **common) == hip.ERR_ARG
    assert hip.call("ditto_guided_step_packed_multistep_project_opts", q=P, step=None, coefs=P, **common) == hip.ERR_ARG
