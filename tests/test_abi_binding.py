"""The typed binding of the C ABI (bipedal_control_amd/abi.py): every prototype of include/bpmpc.h is parsed, what is declared is what libbpmpc.so
exports, one signature per kind of the type mapping is what it reads in C, all struct mirrors match the header's members, a mistyped call raises
before it reaches C and a plain Python float is a double.  No GPU."""
import ctypes as C
import ctypes.util
import re
import shutil
import subprocess

import numpy as np
import pytest

from bipedal_control_amd import abi, load_library
from bipedal_control_amd.api import library_path

DP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int)


def test_the_parser_skips_nothing():
    protos = abi.prototypes(abi.HEADER)
    assert len(protos) == len(re.findall(r"\bbpmpc_\w+\s*\(", abi.declarations(abi.HEADER))) and len(protos) > 0
    for name, (ret, params) in protos.items():
        assert ret in ("int", "void", "const char*"), (name, ret)
        assert all(params), name


def test_declared_equals_exported():
    lib, protos = load_library(), abi.prototypes(abi.HEADER)
    for name in protos:
        assert hasattr(lib, name), "libbpmpc.so does not export " + name
    if shutil.which("nm") is None:
        pytest.skip("nm is missing: the exported symbols cannot be listed")
    out = subprocess.run(["nm", "-D", "--defined-only", library_path()], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split() and line.split()[-1].startswith("bpmpc_")}
    assert exported and exported <= set(protos), sorted(exported - set(protos))


def test_spot_signatures():
    lib = load_library()
    V, VP = C.c_void_p, C.POINTER(C.c_void_p)
    expected = {
        "bpmpc_solver_read": (C.c_int, [V, C.c_char_p, DP, C.c_long]),
        "bpmpc_solver_device_trajectories": (C.c_int, [V, C.POINTER(DP), C.POINTER(DP)]),
        "bpmpc_cmd_vel_to_targets": (C.c_int, [V, DP, C.c_double, DP, C.c_double, DP, DP]),
        "bpmpc_model_joint_name": (C.c_int, [V, C.c_int, C.c_char_p, C.c_int]),
        "bpmpc_plant_step": (C.c_int, [V, C.c_int, C.POINTER(abi._JointCommand), C.c_int, C.c_double, C.c_int]),
        "bpmpc_solver_create": (C.c_int, [V, C.POINTER(abi._Settings), VP]),
        "bpmpc_solver_destroy": (None, [V]),
        "bpmpc_last_error": (C.c_char_p, []),
    }
    for name, (restype, argtypes) in expected.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name


def _members(body):
    """[(name, ctypes type)] of a struct body: `double *a, *b;`, `const int* modes;`, `void* stream;`, `bpmpc_sensor_inputs sensors;`"""
    out = []
    for decl in filter(None, (" ".join(d.split()) for d in body.split(";"))):
        base, rest = re.fullmatch(r"(?:const )?(\w+)\b(.*)", decl).groups()
        for item in rest.split(","):
            stars, name = re.fullmatch(r"\s*(\**)\s*(\w+)", item).groups()
            t = {"int": C.c_int, "double": C.c_double, "void": None}[base] if base not in abi.MIRRORS else abi.MIRRORS[base]
            for _ in stars:
                t = C.POINTER(t) if t is not None else C.c_void_p
            assert t is not None, decl
            out.append((name, t))
    return out


def test_struct_mirrors_match_the_header():
    structs = re.findall(r"typedef\s+struct\s*\{([^}]*)\}\s*(bpmpc_\w+)\s*;", abi.declarations(abi.HEADER))
    assert {name for _, name in structs} == set(abi.MIRRORS) and len(structs) == len(abi.MIRRORS)
    for body, name in structs:
        assert _members(body) == list(abi.MIRRORS[name]._fields_), name


def test_mistyped_calls_never_reach_c():
    lib = load_library()
    d, i, n = (C.c_double * 32)(), (C.c_int * 32)(), C.c_int()
    wrong = (C.ArgumentError, TypeError)
    with pytest.raises(wrong):                                 # an int array where const double* event_times is declared
        lib.bpmpc_time_grid(0.0, 1.0, 0.1, i, 0, d, i, 32, C.byref(n))
    with pytest.raises(wrong):                                 # a float where int n_events is declared
        lib.bpmpc_time_grid(0.0, 1.0, 0.1, d, 0.0, d, i, 32, C.byref(n))
    with pytest.raises(wrong):                                 # n_nodes is missing
        lib.bpmpc_time_grid(0.0, 1.0, 0.1, d, 0, d, i, 32)
    assert lib.bpmpc_time_grid(0.0, 1.0, 0.1, d, 0, d, i, 32, C.byref(n)) == 0 and n.value >= 10          # the same call, typed as declared, arrives


def test_a_python_float_is_a_double():
    lib = load_library()
    ev = np.array([0.35, 0.7])

    def grid(wrap):
        t, e, n = np.zeros(256), np.zeros(256, np.int32), C.c_int()
        assert lib.bpmpc_time_grid(wrap(0.1), wrap(1.0), wrap(0.015), ev.ctypes.data_as(DP), 2, t.ctypes.data_as(DP), e.ctypes.data_as(IP), 256, C.byref(n)) == 0
        return t[:n.value], e[:n.value]

    plain, wrapped = grid(float), grid(C.c_double)
    assert len(plain[0]) >= 60 and np.array_equal(plain[0], wrapped[0]) and np.array_equal(plain[1], wrapped[1])
    assert 1 in plain[1] and 2 in plain[1]                      # the grid saw both events


def test_bind_is_strict_about_missing_exports():
    libm = C.CDLL(ctypes.util.find_library("m"))
    with pytest.raises(AttributeError):
        abi.bind(libm)
    assert abi.bind(libm, strict=False) is libm
    assert not any(name.startswith("bpmpc_") for name in vars(libm))
    assert libm.cos.argtypes is None


def test_an_unmapped_declaration_is_an_error(tmp_path):
    header = tmp_path / "other.h"
    header.write_text("/* not a type of the mapping */\nint bpmpc_version(float x);\n")
    with pytest.raises(TypeError, match="float x"):
        abi.bind(C.CDLL(ctypes.util.find_library("m")), strict=False, header_path=str(header))


def test_a_missing_header_is_an_error(monkeypatch, tmp_path):
    from bipedal_control_amd import api
    monkeypatch.setattr(api, "_LIB", None)
    monkeypatch.setattr(abi, "HEADER", str(tmp_path / "absent.h"))
    with pytest.raises(api.BpmpcError, match="bpmpc.h is missing"):
        api.load_library()
