"""The whole boundary between include/gmpe.h, libgmpe.so and their ctypes mirror (gmpe/_lib.py, gmpe/config.py), table-driven from tests/abi_lib.py: a
struct, constant, entry point or kernel is covered the moment it exists. No GPU.
  - every mirror struct: sizeof and every field's offset and size are the header's; header structs and mirrors are the same set;
  - every GMPE_* #define / enumerator has its value in its mirror, or stands in UNMIRRORED / one of the named ties below;
  - _lib.SYMBOLS are the header's functions, each exported by the library and bound;
  - every prototype's parameters against the argtypes _lib.load() sets;
  - every kernel of every object of the Makefile's RUFILES uses no scratch (the fused kernel's allow-list is tests/test_host_logic.py's)."""
import ctypes as C
import re

import pytest

import abi_lib as A
from gmpe import _lib
from gmpe import config as gcfg
from gmpe import evaluate as EV

MIRRORS = A.mirrors()


@pytest.mark.parametrize("cls,cname", MIRRORS, ids=[n for _, n in MIRRORS])
def test_struct_layout_is_the_headers(cls, cname):
    assert cname in A.struct_names()
    assert A.mirror_layout(cls) == A.layout(cls)


def test_header_structs_and_mirrors_are_the_same_set():
    assert sorted(n for _, n in MIRRORS) == A.struct_names()
    assert sorted(A.enumerators()) == ["gmpe_dynamics", "gmpe_field", "gmpe_formation", "gmpe_scenario", "gmpe_status"]      # the header's other typedefs
    print("structs %d, fields %d" % (len(MIRRORS), sum(len(c._fields_) for c, _ in MIRRORS)))


# Header constants whose mirror has another name, or none. Everything else must be an upper-case name of _lib or config with GMPE_ taken off.
TIED = {"GMPE_PPO_OUT_" + k.upper(): i for i, k in enumerate(_lib.PPO_OUT)}                                # columns of gmpe_ppo_loss' `out`
TIED.update({"GMPE_EVAL_" + {"total_dists_traveled": "TOTAL_DISTS", "total_time_taken": "TOTAL_TIME"}.get(c, c.upper()): i for i, c in enumerate(EV.COLUMNS)})
TIED.update({"GMPE_EVAL_STAT_" + s.upper(): i for i, s in enumerate(EV.STATS)})
TIED.update({"GMPE_F_" + k.upper(): v[0] for k, v in gcfg.FIELDS.items()})                                 # gmpe_field against config.FIELDS
TIED["GMPE_F_COUNT"] = len(gcfg.FIELDS)
TIED.update({"GMPE_FORMATION_" + k.upper(): v for k, v in gcfg.FORMATIONS.items()})
TIED["GMPE_INFO_KEYS"] = len(gcfg.INFO_KEYS)                                                                # config.INFO_KEYS is the list itself
UNMIRRORED = {
    # gmpe_status: Python sees a non-zero return code and the text of gmpe_last_error (_lib.check); tests compare with the literals
    "GMPE_OK": 0, "GMPE_ERR_INVALID_ARG": -1, "GMPE_ERR_HIP": -2, "GMPE_ERR_NO_DEVICE": -3, "GMPE_ERR_UNSUPPORTED": -4, "GMPE_ERR_TAPE_EXHAUSTED": -5,
    "GMPE_ERR_PLACEMENT": -6,
    # limits gmpe_create enforces; config.py restates neither
    "GMPE_MAX_AGENTS": 64, "GMPE_MAX_ENTITIES": 160,
}
# GMPE_H, the include guard, has no value and is no constant.


def _mirrored(name):
    short = name[len("GMPE_"):]
    return [getattr(m, short) for m in (_lib, gcfg) if short.isupper() and isinstance(getattr(m, short, None), int)]


def test_every_header_constant_has_its_value_in_the_mirror():
    names = A.header_constants()
    assert len(names) == len(set(names)) and "GMPE_H" not in names
    by_name, tied, unmirrored = 0, 0, 0
    for n in names:
        got = _mirrored(n)
        if got:
            assert n not in TIED and n not in UNMIRRORED, n
            assert got == [A.constant(n)] * len(got), n
            by_name += 1
        elif n in TIED:
            assert TIED[n] == A.constant(n), n
            tied += 1
        else:
            assert n in UNMIRRORED, "%s of include/gmpe.h has no mirror in _lib / config and is not listed here" % n
            assert UNMIRRORED[n] == A.constant(n), n
            unmirrored += 1
    assert not (set(TIED) | set(UNMIRRORED)) - set(names)                     # nothing listed here that the header no longer has
    print("constants %d: %d by name, %d tied, %d unmirrored" % (len(names), by_name, tied, unmirrored))


def test_symbols_are_the_headers_exported_and_bound():
    lib = _lib.load()
    assert sorted(_lib.SYMBOLS) == A.declared_functions() == sorted(n for _, n, _ in A.prototypes()) and len(_lib.SYMBOLS) >= 15
    for f in _lib.SYMBOLS:
        assert f in A.exported(), "libgmpe.so does not export %s declared in include/gmpe.h" % f
        assert hasattr(lib, f), f
    assert lib.gmpe_abi_version() == gcfg.ABI_VERSION == A.constant("GMPE_ABI_VERSION")


EXACT = {"int64_t": C.c_int64, "uint64_t": C.c_uint64, "size_t": C.c_size_t, "float": C.c_float, "double": C.c_double}
BY_C_NAME = {n: c for c, n in MIRRORS}


def _check_parameter(ctype, bound):
    base = re.sub(r"^const\s+", "", ctype)
    if base.endswith("*"):
        if bound is C.c_void_p:
            return
        assert issubclass(bound, C._Pointer), bound
        to, pointee = bound._type_, base[:-1]
        if issubclass(to, C.Structure):
            assert BY_C_NAME.get(pointee) is to, (pointee, to)
        else:                                                               # out-parameters: size_t*, double*, int64_t*, handle / pointer **
            assert to is (C.c_void_p if pointee.endswith("*") else EXACT[pointee]), (pointee, to)
    elif base in ("int", "int32_t"):
        assert issubclass(bound, C._SimpleCData) and bound._type_ in "il" and C.sizeof(bound) == 4, bound
    else:
        assert bound is EXACT[base], (base, bound)


def test_argtypes_are_the_headers_prototypes():
    lib = _lib.load()
    protos = A.prototypes()
    assert len(protos) == len(_lib.SYMBOLS)
    n_params = 0
    for ret, name, params in protos:
        fn = getattr(lib, name)
        if fn.argtypes is None:
            assert not params, "%s has %d parameters and no argtypes" % (name, len(params))
        else:
            assert len(fn.argtypes) == len(params), name
            for i, (ctype, bound) in enumerate(zip(params, fn.argtypes)):
                try:
                    _check_parameter(ctype, bound)
                except (AssertionError, KeyError) as e:
                    raise AssertionError("%s parameter %d (%s) is bound as %s: %r" % (name, i, ctype, bound, e))
        if ret == "const char*":
            assert fn.restype is C.c_char_p, name
        else:
            assert ret == "int" and fn.restype is C.c_int, (name, ret)
        n_params += len(params)
    print("prototypes %d, parameters %d" % (len(protos), n_params))


def test_no_kernel_uses_scratch():
    """Every kernel of every RUFILES object reports zero bytes of scratch; the fused kernel's instantiations are held to their allow-list by
    tests/test_host_logic.py::test_kernels_do_not_spill."""
    ru = A.resource_usage()
    assert list(ru) == A.ru_objects() and all(ru.values())
    bad = [(o, k, x) for o in ru for k, x in A.scratch(o).items() if "k_env" not in k and x != 0]
    assert not bad, bad
    print("kernels %d in %d objects, %d of them k_env" % (sum(len(k) for k in ru.values()), len(ru), sum("k_env" in k for ks in ru.values() for k in ks)))
    print("child processes:", A.RUNS)
