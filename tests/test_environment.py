"""CPU tests of the environment radiance (spt_set_environment): the header and the libraries declare and export it, the Python front
validates E before any device call, the optional "environment" key of a scene file round-trips through scene.py and through the C++
loader / writer (absent = black), and smallpt_cli's --env parses and overrides the file."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "smallpt_mi355x.h")
MULTI_HEADER = os.path.join(ROOT, "include", "smallpt_mi355x_multi.h")
CLI = os.path.join(ROOT, "optix-test-smallpt_amd", "host", "smallpt_mi355x")


def test_header_declares_environment_entry_points():
    text = open(HEADER).read()
    assert re.search(r"int\s+spt_set_environment\(spt_ctx\* ctx, const float radiance\[3\]\);", text)
    assert re.search(r"int\s+spt_get_environment\(const spt_ctx\* ctx, float radiance\[3\]\);", text)
    assert "Enclosure anchor" in text and "smallpt.cpp:168" in text
    assert re.search(r"int\s+spt_multi_set_environment\(spt_multi\* m, const float radiance\[3\]\);", open(MULTI_HEADER).read())


def test_libraries_export_environment_entry_points(pkg):
    lib = C.CDLL(pkg.LIB_PATH)
    for name in ("spt_set_environment", "spt_get_environment"):
        assert hasattr(lib, name) and name in pkg.SYMBOLS
    multi = C.CDLL(os.path.join(os.path.dirname(pkg.LIB_PATH), "libsmallpt_mi355x_multi.so"))
    assert hasattr(multi, "spt_multi_set_environment") and "spt_multi_set_environment" in pkg.MULTI_SYMBOLS
    assert lib.spt_set_environment(None, None) == 1                  # NULL context: refused without a device


@pytest.mark.parametrize("bad", [(1.0, float("nan"), 0.0), (float("inf"), 0.0, 0.0), (0.0, -0.5, 1.0), (1.0, 2.0), (1.0, 2.0, 3.0, 4.0),
                                 [[1.0, 2.0, 3.0]], (-float("inf"), 1.0, 1.0)])
def test_python_validation_rejects(pkg, bad):
    with pytest.raises(ValueError):
        pkg.environment_radiance(bad)


def test_python_validation_accepts(pkg):
    assert pkg.environment_radiance(None).tolist() == [0.0, 0.0, 0.0]
    e = pkg.environment_radiance([0.3, 0, 1e30])
    assert e.dtype == np.float32 and e.tolist() == [np.float32(0.3), 0.0, np.float32(1e30)]
    assert pkg.environment_radiance((-0.0, 0.0, 0.0)).tolist() == [0.0, 0.0, 0.0]


def test_scene_py_roundtrip(pkg):
    sc = pkg.cornell9()
    text = pkg.spheres_to_json(sc, environment=(0.3, 0.7, 1.9))
    assert pkg.environment_from_json(text).tobytes() == np.array([0.3, 0.7, 1.9], np.float32).tobytes()
    back, _ = pkg.spheres_from_json(text)
    assert back.tobytes() == sc.tobytes()
    assert pkg.environment_from_json(pkg.spheres_to_json(sc)).tolist() == [0, 0, 0]           # absent key: black
    assert "environment" not in json.loads(pkg.spheres_to_json(sc))
    meshes = [pkg.make_sphere_trimesh((0, 0, 0), 1.0, 4)]
    mats = [((0, 0, 0), (.5, .5, .5), pkg.DIFF)]
    mt = pkg.meshes_to_json(meshes, mats, generators=[((0, 0, 0), 1.0, 4)], environment=(2, 0, 0.25))
    assert pkg.environment_from_json(mt).tolist() == [2, 0, 0.25]
    assert len(pkg.meshes_from_json(mt)[0]) == 1
    with pytest.raises(ValueError):
        pkg.environment_from_json('{"spheres": [], "environment": [1, 2]}')


def _build_cli():
    subprocess.check_call(["make", "-C", os.path.dirname(CLI), "-s"])


def _cli_env(*args):
    out = subprocess.check_output([CLI, *args, "--print-environment"]).decode().split()
    assert out[0] == "environment"
    return np.array([float(v) for v in out[1:]], dtype=np.float32)


def test_cpp_loader_and_writer_roundtrip(pkg, tmp_path):
    _build_cli()
    sc = pkg.cornell9()
    env = np.array([0.3, 0.7, 1.9], np.float32)
    p = tmp_path / "scene.json"
    p.write_text(pkg.spheres_to_json(sc, environment=env))
    assert _cli_env("--scene", str(p)).tobytes() == env.tobytes()
    raw = subprocess.check_output([CLI, "--scene", str(p), "--parse-only"])
    assert raw == sc.tobytes()                                                               # the key does not disturb the table
    q = tmp_path / "dump.json"
    subprocess.check_call([CLI, "--scene", str(p), "--dump-scene", str(q), "--parse-only"], stdout=subprocess.DEVNULL)
    assert pkg.environment_from_json(q.read_text()).tobytes() == env.tobytes()               # C++ writer -> Python reader
    assert _cli_env("--scene", str(q)).tobytes() == env.tobytes()                            # C++ writer -> C++ reader
    p0 = tmp_path / "plain.json"
    p0.write_text(pkg.spheres_to_json(sc))
    assert _cli_env("--scene", str(p0)).tolist() == [0, 0, 0]                                # absent: black
    assert _cli_env().tolist() == [0, 0, 0]                                                  # built-in Cornell-9
    q0 = tmp_path / "dump0.json"
    subprocess.check_call([CLI, "--scene", str(p0), "--dump-scene", str(q0), "--parse-only"], stdout=subprocess.DEVNULL)
    assert "environment" not in json.loads(q0.read_text())


def test_cpp_loader_rejects_bad_environment(pkg, tmp_path):
    _build_cli()
    for bad in ("[1, 2]", "[1, -2, 3]", "\"sky\""):
        p = tmp_path / "bad.json"
        p.write_text('{"spheres": [], "environment": %s}' % bad)
        r = subprocess.run([CLI, "--scene", str(p), "--print-environment"], capture_output=True)
        assert r.returncode == 1 and b"environment" in r.stderr, bad


def test_cli_env_option(pkg, tmp_path):
    _build_cli()
    assert _cli_env("--env", "0.5,1,2").tolist() == [0.5, 1, 2]
    p = tmp_path / "scene.json"
    p.write_text(pkg.spheres_to_json(pkg.cornell9(), environment=(3, 3, 3)))
    assert _cli_env("--scene", str(p), "--env", "0,0.25,0").tolist() == [0, 0.25, 0]       # --env overrides the file
    for bad in ("1,2", "1,-1,0", "a,b,c", "inf,0,0"):
        r = subprocess.run([CLI, "--env", bad, "--print-environment"], capture_output=True)
        assert r.returncode == 2 and b"--env" in r.stderr, bad
