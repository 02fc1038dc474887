"""CPU-only: the C-ABI library loads, exports every symbol include/tpg.h declares, the Python binding declares every
prototype as the header does, and the library fails loudly (no CPU fallback) when no HIP device is usable."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_symbols():
    txt = open(os.path.join(ROOT, "include", "tpg.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(tpg_[A-Za-z0-9_]+)\s*\(", txt)))


def test_library_exports_every_declared_symbol():
    from tidypopgen_amd import _lib

    syms = _header_symbols()
    assert len(syms) >= 40
    missing = [s for s in syms if not hasattr(_lib.lib, s)]
    assert not missing, missing
    assert sorted(_lib.SYMBOLS) == syms  # the python binding lists exactly the header's surface


# The ctypes spelling of a C type of include/tpg.h (the rule _lib.PROTOTYPES follows).  A scalar by value has the ctypes type
# of its width.  Every pointer is a c_void_p -- pointer to a scalar, opaque handle, handle out-parameter, and the char* output
# buffer of tpg_prof_dump; that includes the double* of tpg_tajimas_d_from_sums and the int64_t* of tpg_ld_band_links -- except
# a const char* (c_char_p), a pointer to a struct the binding mirrors (POINTER(Struct)) and the allreduce callback.
_SCALARS = {"int": C.c_int, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "size_t": C.c_size_t,
            "double": C.c_double}
_POINTEES = {"void", "char", "int", "int32_t", "int64_t", "uint8_t", "uint32_t", "double",
             "tpg_ctx", "tpg_fbm", "tpg_view", "tpg_pairwise", "tpg_comm", "tpg_multi", "tpg_stream", "tpg_roh"}
_STRUCTS = {"tpg_stream_job": "StreamJob", "tpg_stream_qc_job": "StreamQcJob", "tpg_stream_report": "StreamReport",
            "tpg_impute_report": "ImputeReport", "tpg_ld_report": "LdReport", "tpg_roh_params": "RohParams",
            "tpg_f2_params": "F2Params", "tpg_admix_params": "AdmixParams"}
_CALLBACK = "int (*allreduce)(void* user, void* buf, int64_t count, int dtype)"


def _ctype(_lib, decl, is_return=False):
    """one parameter declaration ("const int32_t* rowInd1") or return type -> the ctypes type the rules give it"""
    if decl == _CALLBACK:
        return _lib.HOST_ALLREDUCE
    m = re.fullmatch(r"(const\s+)?(\w+)\s*(\**)\s*(\w*)", decl)
    assert m, f"a declaration the rules do not cover: {decl!r}"
    const, base, stars, name = m.groups()
    assert is_return or name, f"a parameter without a name: {decl!r}"
    if not stars:
        if is_return and base == "void":
            return None
        assert base in _SCALARS, f"a C type the rules do not cover: {decl!r}"
        return _SCALARS[base]
    if base == "char" and const and stars == "*":
        return C.c_char_p
    if base in _STRUCTS and stars == "*":
        return C.POINTER(getattr(_lib, _STRUCTS[base]))
    assert base in _POINTEES and len(stars) <= 2, f"a C type the rules do not cover: {decl!r}"
    return C.c_void_p


def _header_prototypes(_lib):
    """name -> (restype, argtypes) of every function include/tpg.h declares, in header order"""
    txt = open(os.path.join(ROOT, "include", "tpg.h")).read()
    txt = re.sub(r"/\*.*?\*/", " ", txt, flags=re.S)
    protos = {}
    for ret, name, params in re.findall(r"^((?:const\s+)?\w+\s*\**)\s*\b(tpg_\w+)\s*\(((?:[^()]|\([^()]*\))*)\)\s*;", txt, flags=re.M):
        params = " ".join(params.split())
        # (commas inside the callback's own parameter list do not separate parameters)
        parts = [p.strip().replace("\0", ",") for p in re.sub(r"\([^()]*\)", lambda m: m.group(0).replace(",", "\0"), params).split(",")]
        args = [] if parts == ["void"] else [_ctype(_lib, p) for p in parts]
        assert name not in protos, name
        protos[name] = (_ctype(_lib, " ".join(ret.split()), is_return=True), args)
    return protos


def test_binding_declares_every_prototype_as_the_header_does():
    from tidypopgen_amd import _lib

    want = _header_prototypes(_lib)
    assert sorted(want) == _header_symbols()  # the prototype regex misses no function; the cap on functions left out is zero
    assert list(_lib.PROTOTYPES) == list(want)  # no entry the header lacks, none missing, header order
    wrong = {}
    for name, (restype, argtypes) in want.items():
        fn = getattr(_lib.lib, name)
        got = (fn.restype, list(fn.argtypes) if fn.argtypes is not None else None)
        if got != (restype, argtypes):
            wrong[name] = got
    assert not wrong, wrong


def _cut_by_size_narrow_blocks(m, block_size):
    """blocks narrower than the widest when CutBySize(m, block_size) cuts m loci (R/local_reimplementations.R:13-15):
    nb = ceiling(m / block_size) blocks, block b ends at round(b m / nb), half to even (Python's round on a float)"""
    nb = -(-m // block_size)
    ends = [0] + [int(round((b + 1) * (m / nb))) for b in range(nb)]
    sizes = [e1 - e0 for e0, e1 in zip(ends, ends[1:])]
    return sum(sz < max(sizes) for sz in sizes)


def test_int64_arguments_are_not_cut_to_32_bits():
    # bare Python ints above 2^32 through two host-only entry points (no device, no context).  Without a prototype ctypes
    # passes a bare int as a C int, and the library would see the low 32 bits: (5, 2^20) and 5 below
    from tidypopgen_amd import _lib

    lib = _lib.lib
    m, bs = (1 << 33) + 5, (1 << 32) + (1 << 20)  # two blocks of 2^32 + 2 and 2^32 + 3 loci: one is narrower
    want, want_cut = _cut_by_size_narrow_blocks(m, bs), _cut_by_size_narrow_blocks(m & 0xFFFFFFFF, bs & 0xFFFFFFFF)
    assert (want, want_cut) == (1, 0)  # the cut arguments give one block of 5 loci: the case tells the two apart
    assert lib.tpg_as_pad_quirk_blocks(m, bs) == want
    assert lib.tpg_as_pad_quirk_blocks(m & 0xFFFFFFFF, bs & 0xFFFFFFFF) == want_cut

    # tpg_shard_loci: the int64 comes back through int64_t* out-parameters; shards tile [0, m) on multiples of 128 loci
    groups = -(-m // 128)
    edges = [min(groups * r // 2 * 128, m) for r in range(3)]
    assert edges[2] == m > 1 << 32
    for rank in range(2):
        b, e = C.c_int64(), C.c_int64()
        assert lib.tpg_shard_loci(m, 2, rank, C.byref(b), C.byref(e)) == 0
        assert (b.value, e.value) == (edges[rank], edges[rank + 1])


def test_no_cpu_fallback_without_device():
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    import tidypopgen_amd as tpg

    with pytest.raises(tpg._lib.TpgError) as e:
        tpg.Context(0)
    assert "no HIP device" in str(e.value) or "hip" in str(e.value).lower()


def test_product_does_not_import_the_oracle():
    # the oracle is test infrastructure: nothing under tidypopgen_amd/ may reference it
    pkg = os.path.join(ROOT, "tidypopgen_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                src = open(os.path.join(dirpath, f)).read()
                assert "import oracle" not in src and "from oracle" not in src and "tpg_oracle" not in src.replace(
                    "oracle/tpg_oracle.c: orc_synth_fbm", ""), f
