"""The clean groups next to the bit per text position (sub_group; kbo_amd/csrc/map_subst.hpp), on the host.  tools/map_group_check.cpp
takes random position bitmaps and bitmaps with planted runs at the sizes the device copy allocates for texts of 200 - 3 000 positions,
makes the group array with the header's group_word(), and checks (1) that every group bit is the AND of its four position bits, both
ends of the array included; (2) that the header's in-window test on ONE 8-byte load equals the position's group bit read the plain way,
for every alignment of q0 (0 .. 31), every read length 3 - 160 and every base, over the first and the last possible diagonal, with every
byte of the load inside array + slack at the bound the header states; (3) that the t-th-unsettled mapping equals counting, for every
13-bit mask and every t.  With the AND replaced by an OR (--break) the program has to fail.  A stand-alone program under
AddressSanitizer and UBSan.  No GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("map_group") / "map_group_check")
    subprocess.run(["c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I",
                    os.path.join(ROOT, "kbo_amd", "csrc"), os.path.join(ROOT, "tools", "map_group_check.cpp"), "-o", path], check=True)
    return path


def test_group_bits_window_test_and_mapping(exe):
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "every index in range" in run.stdout and "every group bit is the AND of its position bits" in run.stdout
    assert "the in-window test reads the position's group bit" in run.stdout and "the mapping finds the t-th entry left" in run.stdout


def test_the_check_fails_when_the_and_is_an_or(exe):
    run = subprocess.run([exe, "--break"], capture_output=True, text=True)
    assert run.returncode == 1, run.stdout + run.stderr
    assert "A GROUP BIT IS NOT THE AND OF ITS POSITION BITS" in run.stdout and "every index in range" in run.stdout
