"""lds_image.h's shading-table text -- what rt_scene_update_materials / _textures' derive pass shares with the LDS scene
image's builder -- built with g++ and checked on the host (tests/native/lds_material_check.cpp): image_put_material's
entries against the values restated here in numpy float64 (one IEEE operation per operator, as -ffp-contract=off gives),
compared as bits, and image_material_entries' first-encounter-in-slot-order assignment for a small slot sequence."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAT_CAP, CHECKER = 512, 0x8000  # layout.h kLdsMatCap, kLdsMatChecker


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = tmp_path_factory.mktemp("lds_material") / "lds_material_check"
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "another_raytracer_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "lds_material_check.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout
    entries, codes = {}, []
    for line in out.stdout.splitlines():
        w = line.split()
        if w[0] == "entry":
            entries.setdefault(w[1], []).append((int(w[2]), np.array([int(x, 16) for x in w[3:7]], np.uint64).view(np.float64)))
        elif w[0] == "codes":
            codes.append([int(x) for x in w[1:]])
        elif w[0] == "nent":
            codes[-1] = (codes[-1], int(w[1]), int(w[3]))
    return entries, codes


def same_bits(got, want):
    return (np.asarray(got, np.float64).view(np.int64) == np.asarray(want, np.float64).view(np.int64)).all()


def test_solid_and_checker_entries_hold_the_textures_colours(model):
    entries, _ = model
    (e, v), = entries["solid"]
    assert e == 7 and same_bits(v, [0.125, 0.3, 0.7, 0.0])
    (e, v), = entries["light"]
    assert e == 0 and same_bits(v, [4.0, 5.5, 7.25, 0.0])
    (e0, even), (e1, odd) = entries["checker"]
    assert (e0, e1) == (40, 41)  # even at e, odd at e + 1
    assert same_bits(even, [0.125, 0.3, 0.7, 0.0]) and same_bits(odd, [0.9, 0.1, 1e-3, 0.0])
    # a pair whose odd entry would lie past the table: the even one alone (the program checks that nothing else changed)
    (e, v), = entries["checker_at_the_end"]
    assert e == MAT_CAP - 1 and same_bits(v, [0.125, 0.3, 0.7, 0.0])


def test_metal_entries_hold_albedo_and_fuzz(model):
    entries, _ = model
    (e, v), = entries["metal"]
    assert e == 3 and same_bits(v, [0.7, 0.6, 0.5, 0.25])
    (e, v), = entries["metal_clamped"]  # fuzz 1.5, clamped to 1 by the caller: the entry holds what the record holds
    assert e == MAT_CAP - 1 and same_bits(v, [0.7, 0.6, 0.5, 1.0])


@pytest.mark.parametrize("name,e,ir", [("glass_1.5", 11, 1.5), ("glass_0.75", 12, 0.75)])
def test_dielectric_entries_hold_the_derived_values(model, name, e, ir):
    entries, _ = model
    (got_e, v), = entries[name]
    ir = np.float64(ir)
    one = np.float64(1.0)
    inv = one / ir
    r0f, r0b = (one - inv) / (one + inv), (one - ir) / (one + ir)
    assert got_e == e and same_bits(v, [inv, r0f * r0f, r0b * r0b, ir])
    assert v[1] > 0 and v[2] > 0 and v[0] != ir


def test_entries_are_handed_out_in_first_encounter_slot_order(model):
    _, codes = model
    # slots meet materials 2 (checker: two entries), 3 (dielectric), 2, 2, 1 (metal), 0 (solid), 4 (light), 0; material 5
    # is used by no slot, 6 and 7 are not met
    assert codes[0] == ([4, 3, 0 | CHECKER, 2, 5, -1, -1, -1], 6, 1)
    # a slot of a lambertian over a checker with a noise child, or of an isotropic: no entry for it, the table incomplete
    assert codes[1] == ([4, 3, 0 | CHECKER, 2, 5, -1, -1, -1], 6, 0)
    assert codes[2] == ([4, 3, 0 | CHECKER, 2, 5, -1, -1, -1], 6, 0)
