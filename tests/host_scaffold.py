"""What the host tests of every stage share: the loaded library and its refusals, a stage's config, the result files' names, the CPU
builds of csrc/ headers (a stand-alone program, or a library for ctypes) and the parser that tests/test_host.py holds
include/stac_hip.h against abi.PROTOTYPES with.  A plain module: the fixtures of a test file call it in one line."""

import ctypes as C
import re
import shutil
import subprocess

import numpy as np

from conftest import ROOT

STAC_ERR_INVALID, STAC_ERR_HIP, STAC_ERR_CAPACITY, STAC_ERR_NO_DEVICE = -1, -2, -3, -4
CSRC = ROOT / "stac_mjx_amd" / "csrc"
HEADER = ROOT / "include" / "stac_hip.h"


# ---- the library ---------------------------------------------------------------------------------------------------------------------
def loaded_library():
    from stac_mjx_amd.build import build_extension
    from stac_mjx_amd.engine import load_library

    build_extension()
    return load_library()


def invalid(lib, rc, code=STAC_ERR_INVALID):
    """``rc`` is the refusal ``code``, the library's last error carries it and a text -> the text."""
    msg = lib.stac_last_error().decode()
    assert rc == code and lib.stac_last_error_code() == code and msg, (rc, msg)
    return msg


# ---- config and result files ---------------------------------------------------------------------------------------------------------
def stage_cfg(rodent_cfg, **over):
    from stac_mjx_amd.config import validate_config

    stac = dict(fit_offsets_path="fit.h5", ik_only_path="ik.h5", data_path="d.mat", continuous=False, n_fit_frames=4,
                skip_fit_offsets=False, skip_ik_only=False, infer_qvels=False, n_frames_per_clip=2,
                mujoco=dict(solver="newton", iterations=1, ls_iterations=4))
    stac.update(over)
    return validate_config({"model": dict(rodent_cfg), "stac": stac})


def result_suffixes():
    from stac_mjx_amd import io

    return [".npz"] + ([".h5"] if io.h5py is not None else [])  # (.h5 where h5py is installed; else the writer's .npz stand-in alone)


def dataset_names(path):
    from stac_mjx_amd import io

    if path.suffix == ".npz":
        with np.load(path) as f:
            return set(f.files)
    with io.h5py.File(path, "r") as f:
        return set(f.keys())


# ---- CPU builds of csrc/ headers -----------------------------------------------------------------------------------------------------
def host_cxx():
    cxx = next((c for c in map(shutil.which, ("c++", "g++", "clang++")) if c), None)
    assert cxx, "no host C++ compiler"
    return cxx


def build_cpu_program(tmp_path_factory, stem, source, opt):
    """The executable of the stand-alone program ``source`` (its own main; csrc/ on the include path), built at ``opt``."""
    d = tmp_path_factory.mktemp(f"{stem}_host")
    (d / f"{stem}_cpu.cpp").write_text(source)
    exe = d / f"{stem}_cpu"
    base = [host_cxx(), opt, "-g", "-ffp-contract=off", "-std=c++17", f"-I{CSRC}", str(d / f"{stem}_cpu.cpp"), "-o", str(exe)]
    # with the address and undefined-behaviour sanitizers where the host compiler has their runtimes (a stand-alone CPU program)
    if subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True).returncode != 0:
        subprocess.run(base, check=True, capture_output=True, text=True)
    return exe


def build_cpu_library(tmp_path_factory, stem, source):
    """``source`` (extern "C" functions over csrc/ headers) as a shared library for ctypes: the caller declares its argtypes."""
    d = tmp_path_factory.mktemp(f"{stem}_host")
    (d / "driver.cpp").write_text(source)
    so = d / f"lib{stem}_host.so"
    subprocess.run([host_cxx(), "-O2", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC", f"-I{CSRC}", str(d / "driver.cpp"), "-o", str(so)],
                   check=True, capture_output=True, text=True)
    return C.CDLL(str(so))


def fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float)) if a is not None else None


# ---- the header as the compiler reads it ---------------------------------------------------------------------------------------------
_C_CLASSES = ("int32_t", "int64_t", "float", "double", "void")


def c_class(ctype: str) -> str:
    """A C type of the header as one of: pointer, int32_t, int64_t, float, double, void."""
    if "*" in ctype:
        return "pointer"
    base = ctype.replace("const", " ").split()
    assert len(base) == 1 and base[0] in _C_CLASSES, ctype
    return base[0]


def ctypes_class(t) -> str:
    if t is None:
        return "void"
    if t in (C.c_void_p, C.c_char_p) or issubclass(t, C._Pointer):
        return "pointer"
    return {C.c_int32: "int32_t", C.c_int64: "int64_t", C.c_float: "float", C.c_double: "double"}[t]


def header_prototypes() -> tuple:
    """Every ``ret stac_name(args);`` of include/stac_hip.h -> (name: (class of ret, [(class, name) of every argument]), the number
    of prototype statements: more than the names where one is declared twice)."""
    text = re.sub(r"/\*.*?\*/", " ", HEADER.read_text(), flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    text = "\n".join(ln for ln in text.splitlines() if not ln.lstrip().startswith("#"))
    text = text.replace('extern "C" {', " ")
    text = re.sub(r"(typedef\s+struct\s+\w+|enum)\s*\{[^}]*\}\s*\w*\s*;", " ", text)  # struct and enum bodies
    text = re.sub(r"typedef\s+struct\s+\w+\s+\w+\s*;", " ", text)  # opaque handles
    protos, n = {}, 0
    for stmt in text.split(";"):
        stmt = " ".join(stmt.split())
        if stmt in ("", "}"):  # (the closing brace of extern "C")
            continue
        m = re.fullmatch(r"(.*?)\b(stac_[a-z0-9_]+) ?\((.*)\)", stmt)
        assert m, f"not a prototype: {stmt!r}"  # nothing of the header is passed over in silence
        ret, name, args = m.groups()
        args = [] if args.strip() == "void" else [a.strip() for a in args.split(",")]
        # an argument is its type followed by its name: what is left without the last identifier is the type
        protos[name] = (c_class(ret), [(c_class(re.sub(r"\w+$", "", a)), re.search(r"\w+$", a).group()) for a in args])
        n += 1
    return protos, n
