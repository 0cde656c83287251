"""vb_finalize's host-only analysis (csrc/symbolic.hip) without a GPU: tests/cpp/symbolic_check.cpp is
compiled once with the analysis as host code under AddressSanitizer and UBSan, reads a flat dump of a
problem, runs analyze() and checks the invariants the kernels take on trust (layout, landmarks, tile
pattern and fill, Schur work, both factorization schedules, the solve task lists, the partition).  A
violation prints the failed property and exits 1."""
from __future__ import annotations

import functools
import os
import subprocess

import numpy as np
import pytest

from visual_inertial_bundle_adjustment_amd import synth
from visual_inertial_bundle_adjustment_amd.kinds import NUM_FACTOR_KINDS, NUM_VAR_KINDS, VAR_DATA, factor_num_consts, factor_num_vars

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "visual_inertial_bundle_adjustment_amd", "csrc")
REF = os.path.join(ROOT, "oracle", "_ref")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# host code only, and the sanitizers on the host side only (-Xarch_host): nothing here is built for or run on a GPU
SANITIZE = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
FLAGS = ["-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g", *SANITIZE]
VB_E_ARG, VB_E_UNSUPPORTED = -1, -6  # include/viba_hip.h


@functools.lru_cache(maxsize=None)
def checker():
    """(program, analysis object): compiled once per run"""
    os.makedirs(REF, exist_ok=True)
    obj, main, exe = (os.path.join(REF, n) for n in ("symbolic_host.o", "symbolic_check.o", "symbolic_check"))
    subprocess.check_call([HIPCC, *FLAGS, "-c", os.path.join(CSRC, "symbolic.hip"), "-o", obj])
    subprocess.check_call([HIPCC, *FLAGS, "-c", os.path.join(ROOT, "tests", "cpp", "symbolic_check.cpp"), "-o", main])
    subprocess.check_call([HIPCC, *SANITIZE, "-o", exe, main, obj])
    return exe, obj


def write_dump(path, vars, const, fvars, fivals, fconsts, imu_calib_options=0xFF, n_rs=0):
    """the arrays vb_set_vars / vb_add_factors take, flat: header, per variable kind (count, data, constant
    flags), per factor kind (count, handles, integer values, constants)"""
    with open(path, "wb") as f:
        np.array([0x314d59534256, imu_calib_options, n_rs], np.int64).tofile(f)
        for k in range(NUM_VAR_KINDS):
            v = np.asarray(vars[k], np.float64).reshape(-1, VAR_DATA[k])
            c = np.zeros(len(v), np.uint8) if const[k] is None else np.asarray(const[k], np.uint8)
            np.array([len(v)], np.int64).tofile(f)
            np.ascontiguousarray(v).tofile(f)
            c.tofile(f)
        for k in range(NUM_FACTOR_KINDS):
            fv = np.asarray(fvars[k], np.int32).reshape(-1, factor_num_vars(k))
            iv = np.zeros(len(fv), np.int32) if fivals[k] is None or len(fivals[k]) == 0 else np.asarray(fivals[k], np.int32)
            fc = np.asarray(fconsts[k], np.float64).reshape(-1, factor_num_consts(k))
            assert len(iv) == len(fv) == len(fc)
            np.array([len(fv)], np.int64).tofile(f)
            np.ascontiguousarray(fv).tofile(f)
            iv.tofile(f)
            np.ascontiguousarray(fc).tofile(f)
    return path


def dump_generated(path, p):
    n_rs = 0 if p.rs_offsets is None else len(p.rs_offsets) - 1
    return write_dump(path, p.vars, p.const, p.fvars, p.fivals, p.fconsts, p.imu_calib_options, n_rs)


def dump_scene(path, scene):
    """a tests/small_factor_scenes.py Scene, as its build() hands it to an engine"""
    import hp_small_factors as hp
    vars = [scene.vars.get(k, np.zeros((0, VAR_DATA[k]))) for k in range(NUM_VAR_KINDS)]
    const = [scene.const.get(k) for k in range(NUM_VAR_KINDS)]
    if len(vars[hp.GRAVITY]):
        const[hp.GRAVITY] = np.ones(len(vars[hp.GRAVITY]), np.uint8)
    fvars = [[] for _ in range(NUM_FACTOR_KINDS)]
    fconsts = [[] for _ in range(NUM_FACTOR_KINDS)]
    for k, h, c in scene.factors:
        row = np.zeros(factor_num_consts(k))
        row[:len(c)] = c
        fvars[k].append(h), fconsts[k].append(row)
    return write_dump(path, vars, const, fvars, [None] * NUM_FACTOR_KINDS, fconsts, scene.mask)


@pytest.fixture(scope="module")
def dumps(tmp_path_factory):
    d = tmp_path_factory.mktemp("symbolic")
    made = {}

    def get(name):
        if name not in made:
            import test_landmark_paths_gpu as lp
            if name == "wide260":
                p = lp.wide_problem(260)
            elif name == "wide200":
                p = lp.wide_problem(200)
            elif name == "track-edges":
                p = lp.track_edge_problem()[0]
            elif name == "group-windows":
                p = lp.group_window_problem()
            elif name == "B400":
                p = synth.generate(synth.config("B", n_kf=400, n_lm=12000))
            elif name == "micro":
                import small_factor_scenes
                made[name] = dump_scene(str(d / "micro.bin"), small_factor_scenes.micro_bundle())
                return made[name]
            else:
                p = synth.generate(synth.config(name))
            made[name] = dump_generated(str(d / f"{name}.bin"), p)
        return made[name]

    return get


def check(dump, *args):
    r = subprocess.run([checker()[0], dump, *map(str, args)], capture_output=True, text=True)
    assert r.returncode == 0, f"symbolic_check {' '.join(map(str, args))}:\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    return r.stdout


def streams_part_ways(out):
    """more segments than supernode levels: some level runs on more than one stream"""
    levels, segments = (int(out.split(k)[1].split()[0].rstrip(";")) for k in ("two-column) levels ", " segments "))
    return segments > levels


def test_analysis_object_needs_no_hip_runtime():
    undefined = subprocess.check_output(["nm", "-u", checker()[1]], text=True).split()
    assert not [s for s in undefined if s.lstrip("_").startswith("hip")], undefined


def test_config_a_is_one_part(dumps):
    out = check(dumps("A"))
    assert " parts 1 " in out, out


@pytest.mark.parametrize("args", [(), ("--leaf", 256), ("--cutwin", 0), ("--leaf", 2 ** 62), ("--nosn",),
                                  ("--streams", 1), ("--streams", 2), ("--streams", 3), ("--streams", 4),
                                  # leaf 64: the supernodes' tree branches, so the streams part ways and meet (segDep)
                                  ("--leaf", 64, "--streams", 2), ("--leaf", 64, "--streams", 3),
                                  ("--leaf", 64, "--streams", 4)], ids=lambda a: " ".join(map(str, a)) or "default")
def test_minib_single_handle(dumps, args):
    out = check(dumps("miniB"), *args)
    if args == ("--leaf", 2 ** 62):
        assert " parts 1 " in out, out
    if args == ("--leaf", 256):  # more parts than a tree of depth 2 has (7): world 2 and 4 below have real subtrees
        assert int(out.split(" parts ")[1].split()[0]) > 7, out
    if args == ("--leaf", 64, "--streams", 2):
        assert streams_part_ways(out), out


@pytest.mark.parametrize("world", [1, 2, 4])
@pytest.mark.parametrize("leaf", [1024, 256])
def test_minib_partitioned_every_rank(dumps, world, leaf):
    out = check(dumps("miniB"), "--leaf", leaf, "--world", world)
    assert out.count("ok rank") == world, out


@pytest.mark.parametrize("rank", [0, 1])
def test_minib_landmark_shards(dumps, rank):
    p = synth.generate(synth.config("miniB"))
    from visual_inertial_bundle_adjustment_amd.distributed import shard_bounds
    lb, le = shard_bounds(p, 2)[rank]
    check(dumps("miniB"), "--shard", lb, le, int(rank == 0), "--leaf", 256)


@pytest.mark.parametrize("scene", ["wide260", "wide200", "track-edges", "group-windows", "micro"])
def test_landmark_path_scenes_and_micro_bundle(dumps, scene):
    check(dumps(scene))


def test_config_b_scaled_to_400_rigs(dumps):
    """(config B itself takes ~1 min under the sanitizers)"""
    check(dumps("B400"), "--world", 4)
    assert streams_part_ways(check(dumps("B400"), "--streams", 3))
    check(dumps("B400"), "--streams", 4)


def test_digest_is_printed_and_stable(dumps):
    a = check(dumps("A"), "--digest")
    assert a == check(dumps("A"), "--digest") and "digest " in a


def test_errors_return_code_and_message(dumps, tmp_path):
    p = synth.generate(synth.config("A"))
    bad = [v.copy() for v in p.fvars]
    bad[0][3, 1] = len(p.vars[1]) + 7
    write_dump(str(tmp_path / "unknown.bin"), p.vars, p.const, bad, p.fivals, p.fconsts, p.imu_calib_options)
    check(str(tmp_path / "unknown.bin"), "--expect", VB_E_ARG, "factor references an unknown variable handle")
    const = list(p.const)
    const[8] = np.zeros(len(p.vars[8]), np.uint8)
    write_dump(str(tmp_path / "gravity.bin"), p.vars, const, p.fvars, p.fivals, p.fconsts, p.imu_calib_options)
    check(str(tmp_path / "gravity.bin"), "--expect", VB_E_UNSUPPORTED, "non-constant gravity is not supported")
    n_pts = int(np.sum(np.asarray(p.const[0]) == 0))
    check(dumps("A"), "--shard", 0, n_pts + 1, 1, "--expect", VB_E_ARG, "bad landmark shard range")
