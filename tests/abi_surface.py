"""What the test_*_abi.py files share: the library, the flattened text of include/msm_hip.h, the check of a table of prototypes
against the binding, the library and the header, and the frozen ABI version and struct sizes."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "msm_hip.h")


def library():
    from conftest import build_if_missing

    build_if_missing("all", "montgomery_amd/libmsm_hip.so")
    from montgomery_amd import _lib

    return _lib.load()


def header_text():
    return open(HEADER).read()


def flat_header():
    """The header with its comments out and one space between tokens: a prototype reads `int name(type a, type b);`."""
    flat = re.sub(r"/\*.*?\*/", " ", header_text(), flags=re.S)
    return re.sub(r"\s+", " ", flat).replace("( ", "(").replace(" )", ")").replace(" ,", ",")


def assert_prototypes(lib, prototypes):
    """Every name of `prototypes` (name -> the argument list as the header spells it) is bound, is in the library, takes that many
    arguments and returns an int."""
    from montgomery_amd import _lib

    for name, args in prototypes.items():
        assert name in _lib.EXPORTS, name
        fn = getattr(lib, name)                      # AttributeError: the library has no such symbol
        assert len(fn.argtypes) == args.count(",") + 1 and fn.restype is C.c_int, name


def assert_names_declared(names):
    """The check by name alone: the header declares `int name(`, the binding lists it and the library itself exports it."""
    from montgomery_amd import _lib

    text = re.sub(r"/\*.*?\*/", "", header_text(), flags=re.S)
    for n in names:
        assert re.search(r"\bint\s+%s\s*\(" % n, text), f"include/msm_hip.h does not declare {n}"
        assert n in _lib.EXPORTS
    lib = C.CDLL(_lib.LIB_PATH)
    for n in names:
        assert hasattr(lib, n), f"libmsm_hip.so does not export {n}"


def abi_history():
    """The History comment of the header, up to the version's #define."""
    text = header_text()
    return text[text.index("History:"):text.index("#define MSM_ABI_VERSION")]


def assert_header_declares(prototypes):
    """The header declares each prototype token for token, under ABI version 8.  Returns the flattened header."""
    assert re.search(r"#define\s+MSM_ABI_VERSION\s+8\b", header_text())
    flat = flat_header()
    for name, args in prototypes.items():
        assert f"int {name}({args});" in flat, name
    return flat


def assert_abi_frozen(lib):
    """ABI version 8 and the 56- and 176-byte structs, in the library, the binding and the header."""
    from montgomery_amd import _lib

    assert lib.msm_abi_version() == 8 == _lib.ABI_VERSION
    assert lib.msm_abi_struct_bytes(0) == 56 == C.sizeof(_lib.MsmOpts)
    assert lib.msm_abi_struct_bytes(1) == 176 == C.sizeof(_lib.MsmResult)
    assert int(re.search(r"#define\s+MSM_ABI_VERSION\s+(\d+)", header_text()).group(1)) == 8
