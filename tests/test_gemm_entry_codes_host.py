"""Status codes of the seven eval-GEMM entry points (skg_gemm_f32, skg_gemm_group_f32, skg_gemm_b16_f32,
skg_gemm_b16_a16_f32, skg_gemm_group_b16_f32, skg_gemm_b16_x, skg_gemm_group_b16_x) for descriptors that break ONE rule
each: every entry answers with the documented code before anything is launched, and no launch counter moves.  The table
holds rejected or empty descriptors only (a descriptor that passes with M > 0 would try to launch), so it needs no GPU.
The codes were recorded from the library as it stood before the entries shared their launch path."""
import ctypes as C

import pytest

from skghoi_amd import _capi

ARG, ALIGN, LIMIT = -1, -2, -3
SINGLE = ("skg_gemm_f32", "skg_gemm_b16_f32", "skg_gemm_b16_a16_f32", "skg_gemm_b16_x")
GROUPED = ("skg_gemm_group_f32", "skg_gemm_group_b16_f32", "skg_gemm_group_b16_x")
F32 = ("skg_gemm_f32", "skg_gemm_group_f32")
TWIN = tuple(e for e in SINGLE + GROUPED if e not in F32)                    # the entries that take a bf16 weight twin
A16 = ("skg_gemm_b16_a16_f32", "skg_gemm_b16_x", "skg_gemm_group_b16_x")     # ... a bf16 A
X = ("skg_gemm_b16_x", "skg_gemm_group_b16_x")                               # ... a bf16 output
NOT_A16F = tuple(e for e in SINGLE + GROUPED if e != "skg_gemm_b16_a16_f32")
I31 = 2 ** 31 - 1


def _on(entries, code):
    return {e: code for e in entries}


def _every(code):
    return _on(SINGLE + GROUPED, code)


# (what breaks, descriptor fields, io fields, {entry: code}); an entry that is not named does not see the rule (the fp32
# entries take no twin, ...).  Base descriptor and io: _desc() and _io() below.  skg_gemm_b16_a16_f32 gets a16 = 16 where the
# row names none.
CASES = [
    ("A null", dict(A=0), {}, _on(NOT_A16F, ARG)),
    ("A misaligned", dict(A=8), {}, _on(NOT_A16F, ALIGN)),
    ("W null", dict(W=0), {}, _every(ARG)),
    ("W misaligned", dict(W=8), {}, _every(ALIGN)),
    ("w16 null", {}, dict(w16=None), _on(TWIN, ARG)),
    ("w16 misaligned", {}, dict(w16=8), _on(TWIN, ALIGN)),
    ("a16 null", {}, dict(a16=None), {"skg_gemm_b16_a16_f32": ARG}),
    ("a16 misaligned", {}, dict(a16=8), _on(A16, ALIGN)),
    ("C missing", dict(C=0), {}, _every(ARG)),
    ("M < 0", dict(M=-1), {}, _every(ARG)),
    ("N = 0", dict(N=0), {}, _every(ARG)),
    ("K = 0", dict(K=0), {}, _every(ARG)),
    ("K % 4", dict(K=34), {}, _every(ALIGN)),
    ("lda % 4", dict(lda=66), {}, _every(ALIGN)),
    ("ldw % 4", dict(ldw=66), {}, _every(ALIGN)),
    ("ldw % 8 with a twin", dict(ldw=68), {}, _on(TWIN, ARG)),
    ("lda % 8 with a16", dict(lda=68), dict(a16=16), _on(A16, ALIGN)),
    ("K % 8 with a16", dict(K=36), dict(a16=16), _on(A16, ALIGN)),
    ("a_rows with a16", dict(a_rows=16), dict(a16=16), _on(A16, ARG)),
    ("lda < K", dict(lda=16), {}, _every(ARG)),
    ("unknown epilogue", dict(epilogue=5), {}, _every(ARG)),
    ("negative epilogue", dict(epilogue=-1), {}, _every(ARG)),
    ("MUL_RELU without P / Q", dict(epilogue=_capi.EPI_MUL_RELU), {}, _every(ARG)),
    ("RELU_DOT without dot_w", dict(epilogue=_capi.EPI_RELU_DOT, dot_partial=16), {}, _every(ARG)),
    ("RELU_DOT without dot_partial", dict(epilogue=_capi.EPI_RELU_DOT, dot_w=16), {}, _every(ARG)),
    ("RES_RELU without res", dict(epilogue=_capi.EPI_BIAS_RES_RELU), {}, _every(ARG)),
    ("split_k without workspace", dict(split_k=4), {}, _every(ARG)),
    ("split_k = 65", dict(split_k=65, split_ws=16), {}, _every(ARG)),
    ("split_k with MUL_RELU", dict(split_k=4, split_ws=16, epilogue=_capi.EPI_MUL_RELU, P=16), {}, _every(ARG)),
    ("c16 with RELU_DOT", dict(epilogue=_capi.EPI_RELU_DOT, dot_w=16, dot_partial=16), dict(c16=16, ldc16=64), _on(X, ARG)),
    ("ldc16 < N", {}, dict(c16=16, ldc16=3), _on(X, ARG)),
    ("neither C nor c16", dict(C=0), {}, _on(X, ARG)),
    # more than 2^31 - 1 workgroups: a single launch exceeds the limit; a group refuses split-K with 128 x 128 tiles first
    ("oversized grid", dict(M=I31, N=I31, split_k=64, split_ws=16), {}, {**_on(SINGLE, LIMIT), **_on(GROUPED, ARG)}),
    ("oversized grid, ldc16 < N", dict(M=I31, N=I31, split_k=64, split_ws=16), dict(c16=16, ldc16=64), _on(X, ARG)),
    # an empty product passes the checks and launches nothing
    ("M = 0", dict(M=0), {}, _every(0)),
    ("M = 0 with a16 and c16", dict(M=0), dict(a16=16, c16=16, ldc16=64), _on(X, 0)),
    # with a16 given d.A is not read: any value passes (M = 0, so that nothing is launched)
    ("A null beside a16", dict(A=0, M=0), dict(a16=16), _on(A16, 0)),
    ("A misaligned beside a16", dict(A=8, M=0), dict(a16=16), _on(A16, 0)),
]


def _desc(**fields):
    d = _capi.GemmDesc()
    d.A = 16; d.W = 16; d.C = 16; d.lda = 64; d.ldw = 64; d.ldc = 64
    d.M, d.N, d.K, d.epilogue = 4, 4, 32, _capi.EPI_BIAS
    for k, v in fields.items():
        setattr(d, k, v)
    return d


def _io(w16=16, a16=None, c16=None, ldc16=0):
    io = _capi.GemmB16Io()
    io.w16, io.a16, io.c16, io.ldc16 = w16, a16, c16, ldc16
    return io


def _counters():
    """The four launch counters: paths of the eval GEMM, skg_gemm_b16_x's three, the a16 launches, the gemmx paths."""
    lib = _capi.lib()
    p = (C.c_int64 * 4)(); x = (C.c_int64 * 3)(); a = (C.c_int64 * 1)(); g = (C.c_int64 * 3)()
    lib.skg_gemm_path_counts(p, 0); lib.skg_gemm_b16_x_counts(x, 0); lib.skg_gemm_b16_a16_launches(a, 0)
    lib.skg_gemmx_path_counts(g, 0)
    return list(p), list(x), list(a), list(g)


def _call(entry, d, io_fields, pos=0):
    """The status of `entry` for descriptor d; the grouped entries get it first (pos 0) or behind (pos 1) a valid member
    of M == 0."""
    lib = _capi.lib()
    io = _io(**io_fields)
    if entry == "skg_gemm_f32":
        return lib.skg_gemm_f32(C.byref(d), None)
    if entry == "skg_gemm_b16_f32":
        return lib.skg_gemm_b16_f32(C.byref(d), io.w16, None)
    if entry == "skg_gemm_b16_a16_f32":
        return lib.skg_gemm_b16_a16_f32(C.byref(d), io_fields.get("a16", 16), io.w16, None)
    if entry == "skg_gemm_b16_x":
        return lib.skg_gemm_b16_x(C.byref(d), C.byref(io), None)
    arr = (_capi.GemmDesc * 2)(); ios = (_capi.GemmB16Io * 2)(); w16 = (C.c_void_p * 2)()
    arr[pos], ios[pos], w16[pos] = d, io, io.w16
    arr[1 - pos], ios[1 - pos], w16[1 - pos] = _desc(M=0), _io(), 16
    if entry == "skg_gemm_group_f32":
        return lib.skg_gemm_group_f32(arr, 2, None)
    if entry == "skg_gemm_group_b16_f32":
        return lib.skg_gemm_group_b16_f32(arr, w16, 2, None)
    return lib.skg_gemm_group_b16_x(arr, ios, 2, None)


@pytest.mark.parametrize("entry", SINGLE + GROUPED)
def test_one_broken_rule_one_code(entry):
    before = _counters()
    seen = 0
    for what, fields, io_fields, expect in CASES:
        if entry not in expect:
            continue
        for pos in ((0, 1) if entry in GROUPED else (0,)):
            got = _call(entry, _desc(**fields), io_fields, pos)
            assert got == expect[entry], "%s: %s (member %d) -> %d, expected %d" % (entry, what, pos, got, expect[entry])
            seen += 1
    assert seen >= 20
    assert _counters() == before                             # a refused or empty launch moves no counter


def test_null_arguments_and_group_sizes():
    lib = _capi.lib()
    before = _counters()
    d, io = _desc(), _io()
    assert lib.skg_gemm_f32(None, None) == ARG
    assert lib.skg_gemm_b16_f32(None, 16, None) == ARG
    assert lib.skg_gemm_b16_a16_f32(None, 16, 16, None) == ARG
    assert lib.skg_gemm_b16_x(None, C.byref(io), None) == ARG
    assert lib.skg_gemm_b16_x(C.byref(d), None, None) == ARG
    arr = (_capi.GemmDesc * 1)(_desc(M=0)); ios = (_capi.GemmB16Io * 1)(io); w16 = (C.c_void_p * 1)(16)
    big = (_capi.GemmDesc * (_capi.GEMM_GROUP_MAX + 1))()
    bios = (_capi.GemmB16Io * (_capi.GEMM_GROUP_MAX + 1))(); bw16 = (C.c_void_p * (_capi.GEMM_GROUP_MAX + 1))()
    for n, a, i, w in ((1, None, ios, w16), (0, arr, ios, w16), (_capi.GEMM_GROUP_MAX + 1, big, bios, bw16)):
        assert lib.skg_gemm_group_f32(a, n, None) == ARG
        assert lib.skg_gemm_group_b16_f32(a, w, n, None) == ARG
        assert lib.skg_gemm_group_b16_x(a, i, n, None) == ARG
    assert lib.skg_gemm_group_b16_f32(arr, None, 1, None) == ARG
    assert lib.skg_gemm_group_b16_x(arr, None, 1, None) == ARG
    assert lib.skg_gemm_group_f32(arr, 1, None) == 0          # only an empty member: nothing to launch
    assert lib.skg_gemm_group_b16_f32(arr, w16, 1, None) == 0
    assert lib.skg_gemm_group_b16_x(arr, ios, 1, None) == 0
    assert _counters() == before
