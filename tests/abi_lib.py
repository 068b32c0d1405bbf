"""The boundary between include/gmpe.h, libgmpe.so and their hand-written ctypes mirror (gmpe/_lib.py, gmpe/config.py), read once per session:
the header's text, prototypes, structs and constants; every mirror struct with its C name; the values a C compiler gives integer expressions over the
header (one gcc -std=c11 -Wall -Werror run per distinct request); the symbols the library exports; and the compiler's register / scratch report of
every kernel (`make resource-usage`). tests/test_abi_host.py checks all of it table-driven; a feature's host test asks this module for what it says
about its own structs, entry points and kernels. Test infrastructure only: no fixtures, results cached in module globals."""
import ctypes as C
import os
import re
import subprocess
import tempfile

from gmpe import _lib
from gmpe import config as gcfg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "gmpe.h")
CSRC = os.path.join(ROOT, "contracts-marl-aam-corridors_amd", "csrc")
RUNS = {"gcc": 0, "nm": 0, "make": 0}      # child processes started so far, by program
_CACHE = {}


def _once(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


# ---------------------------------------------------------------- the header's text
def header():
    """include/gmpe.h without its comments."""
    return _once("header", lambda: re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S))


def declared_functions():
    return sorted(set(re.findall(r"\b(gmpe_[a-z_0-9]+)\s*\(", header())))


def prototypes():
    """[(return type, name, [parameter C types])] of every function the header declares; a type is written without spaces before its stars."""
    def ctype(text):
        return re.sub(r"\s*\*", "*", " ".join(text.split()))

    def make():
        out = []
        for ret, name, params in re.findall(r"^([A-Za-z_][\w \t\*]*?)\s*\b(gmpe_[a-z_0-9]+)\s*\(([^)]*)\)\s*;", header(), flags=re.M):
            params = [p.strip() for p in params.split(",")]
            out.append((ctype(ret), name, [] if params == ["void"] else [ctype(re.match(r"(.*?)\w+$", p, flags=re.S).group(1)) for p in params]))
        return out
    return _once("prototypes", make)


def struct_names():
    """The structs the header defines (the opaque gmpe_handle has no body)."""
    return sorted(re.findall(r"typedef\s+struct\s+(gmpe_\w+)\s*\{", header()))


def enumerators():
    """{enum name: [its enumerators in order]}."""
    return {name: re.findall(r"\b(GMPE_\w+)", body) for name, body in re.findall(r"typedef\s+enum\s+(gmpe_\w+)\s*\{(.*?)\}", header(), flags=re.S)}


def header_constants():
    """Every GMPE_* #define that has a value and every enumerator, in header order of each kind."""
    return re.findall(r"^[ \t]*#define[ \t]+(GMPE_\w+)[ \t]+\S", header(), flags=re.M) + [e for es in enumerators().values() for e in es]


# ---------------------------------------------------------------- the mirror
def c_name(cls):
    """GmpePpoLossShardPlan -> gmpe_ppo_loss_shard_plan."""
    return re.sub(r"(?<!^)(?=[A-Z])", "_", cls.__name__).lower()


def mirrors():
    """[(ctypes.Structure subclass, its C name)] for every one defined in gmpe._lib and gmpe.config."""
    return [(v, c_name(v)) for m in (gcfg, _lib) for v in vars(m).values()
            if isinstance(v, type) and issubclass(v, C.Structure) and v.__module__ == m.__name__]


# ---------------------------------------------------------------- what a C compiler says
def c_values(expressions):
    """The values of integer C expressions over gmpe.h, from one program compiled as strict C11; one compile per distinct request."""
    def make():
        src = "#include <stdio.h>\n#include <stddef.h>\n#include \"gmpe.h\"\nint main(void) {\n"
        src += "".join("  printf(\"%%lld\\n\", (long long)(%s));\n" % e for e in expressions) + "  return 0;\n}\n"
        with tempfile.TemporaryDirectory() as t:
            cpath, exe = os.path.join(t, "probe.c"), os.path.join(t, "probe")
            with open(cpath, "w") as f:
                f.write(src)
            RUNS["gcc"] += 1
            subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, cpath])
            out = [int(x) for x in subprocess.check_output([exe]).split()]
        assert len(out) == len(expressions)
        return out
    return _once(("c_values",) + tuple(expressions), make)


def _field_expressions(cls, cname):
    return ["sizeof(%s)" % cname] + [e % (cname, f[0]) for f in cls._fields_ for e in ("offsetof(%s, %s)", "sizeof(((%s*)0)->%s)")]


def _table():
    """Every mirror's layout and every header constant in ONE request, so that a session compiles the probe once whatever it asks for."""
    def make():
        exprs = [e for cls, cname in mirrors() if cname in struct_names() for e in _field_expressions(cls, cname)] + header_constants()
        return dict(zip(exprs, c_values(exprs)))
    return _once("table", make)


def layout(cls):
    """(sizeof, {field: (offset, size)}) of the C struct `cls` mirrors, for every field of cls._fields_ by name."""
    v = [_table()[e] for e in _field_expressions(cls, c_name(cls))]
    return v[0], {f[0]: (v[1 + 2 * i], v[2 + 2 * i]) for i, f in enumerate(cls._fields_)}


def mirror_layout(cls):
    """The same shape from ctypes."""
    return C.sizeof(cls), {f[0]: (getattr(cls, f[0]).offset, getattr(cls, f[0]).size) for f in cls._fields_}


def constant(name):
    """The value of a GMPE_* #define or enumerator."""
    return _table()[name]


# ---------------------------------------------------------------- the library
def exported():
    """The defined text symbols of libgmpe.so."""
    def make():
        RUNS["nm"] += 1
        out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
        return {ln.split()[2] for ln in out.splitlines() if len(ln.split()) == 3 and ln.split()[1] == "T"}
    return _once("exported", make)


# ---------------------------------------------------------------- the compiler's report of every kernel
def _makefile_var(text, name):
    return re.search(r"^%s\s*\??=\s*(.*)$" % name, text, flags=re.M).group(1)


def ru_objects():
    """The objects of the Makefile's RUFILES line (build/ru_<object>.txt), in its order."""
    def make():
        text = open(os.path.join(CSRC, "Makefile")).read()
        per_sc, rest = re.match(r"\$\(foreach k,\$\(SCS\),(.*?\.txt)\)(.*)", _makefile_var(text, "RUFILES").replace("$(B)/", "")).groups()
        line = " ".join(per_sc.replace("$(k)", k) for k in _makefile_var(text, "SCS").split()) + rest
        assert "$" not in line, line
        return re.findall(r"\bru_(\w+)\.txt", line)
    return _once("ru_objects", make)


def resource_usage():
    """{object: {mangled kernel name: {"ScratchSize": n, "VGPRs": n, ...}}} from `make resource-usage`, made once per session."""
    def make():
        RUNS["make"] += 1
        out = subprocess.run(["make", "-s", "-C", CSRC, "resource-usage"], capture_output=True, text=True, timeout=900)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
        build = os.path.join(CSRC, _makefile_var(open(os.path.join(CSRC, "Makefile")).read(), "B"))
        ru = {}
        for obj in ru_objects():
            kern = ru[obj] = {}
            for key, val in re.findall(r"remark:\s+([^:\[]+?)(?: \[[^\]]*\])?: (\S+) \[-Rpass-analysis", open(os.path.join(build, "ru_%s.txt" % obj)).read()):
                if key == "Function Name":
                    cur = kern[val] = {}
                else:
                    cur[key] = int(val) if val.isdigit() else val
        return ru
    return _once("resource_usage", make)


def kernels(obj, substring=""):
    """{mangled name: report} of the kernels of one object whose name contains `substring`."""
    return {k: v for k, v in resource_usage()[obj].items() if substring in k}


def scratch(obj, substring=""):
    """{mangled name: bytes of scratch memory per lane} of the same kernels."""
    return {k: v["ScratchSize"] for k, v in kernels(obj, substring).items()}
