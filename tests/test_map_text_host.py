"""The window of the 2-bit text that map_reads_kernel compares a read with (kbo_amd/csrc/map_text.hpp), on the host: the form over the
interleaved text (pc_tm: digits and marks) against the form over the split arrays (pc_t, the summary bits pc_mu, the coarse summary
pc_mc; the marks of marked units alone from pc_tm).  tools/map_text_check.cpp builds random texts of 50 - 2 000 positions with the
padding of pack_text_kernel, plants marks (none, one position, the first and the last position of a unit, two adjacent units, every
unit), packs both layouts and compares every word of the mismatch masks for every diagonal from in front of the text to behind it
(every alignment 0 .. 15), every length 1 .. 160, and stage 2b's three-unit look at both ends of each such window - every array index
through an accessor that checks it against the sizes the device copy allocates.  A stand-alone program under AddressSanitizer and
UBSan.  No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_both_forms_of_the_window_agree_and_stay_in_range(tmp_path):
    exe = str(tmp_path / "map_text_check")
    subprocess.run(["c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I",
                    os.path.join(ROOT, "kbo_amd", "csrc"), os.path.join(ROOT, "tools", "map_text_check.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "every index in range" in run.stdout and "both forms agree" in run.stdout
