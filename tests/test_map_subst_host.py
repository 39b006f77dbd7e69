"""The bit per text position that settles a lone substitution in map_reads_kernel's stage 3 (kbo_amd/csrc/map_subst.hpp), on the host.
tools/map_subst_check.cpp builds random texts of 200 - 3 000 positions over 2 and 4 letters with the padding of pack_text_kernel and
planted marks, takes as the index the set of all strings of `order` bases (4 - 9) of the text, makes the bitmap with the header's
clean() for thresholds order .. order + 8 with and without anchors, and checks, for every position whose bit is set, every other base,
every read length 3 - 160 and the placements of the substitution at both ends of the read, that the entry is eligible and that every
window stage 3 would ask for - the header's offsets, the kernel's own `use` condition, the strings taken from the read - is absent
from the set; that the eligibility predicate accepts a neighbour `order` bases away and rejects one order - 1 away; every index
through an accessor that checks it against the sizes the device copy allocates.  With one window of the proof left out of clean()
the program has to fail.  A stand-alone program under AddressSanitizer and UBSan.  No GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("map_subst") / "map_subst_check")
    subprocess.run(["c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I",
                    os.path.join(ROOT, "kbo_amd", "csrc"), os.path.join(ROOT, "tools", "map_subst_check.cpp"), "-o", path], check=True)
    return path


def test_every_window_of_a_clean_position_is_absent_and_indexes_stay_in_range(exe):
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "every index in range" in run.stdout and "every window of a clean position is absent" in run.stdout
    assert "the predicate holds" in run.stdout


@pytest.mark.parametrize("window", [0, 1, 2, 3])
def test_the_check_fails_when_a_window_is_left_out_of_clean(exe, window):
    run = subprocess.run([exe, "--leave-out", str(window)], capture_output=True, text=True)
    assert run.returncode == 1, run.stdout + run.stderr
    assert "A CLEAN POSITION HAS A PRESENT WINDOW" in run.stdout and "every index in range" in run.stdout
