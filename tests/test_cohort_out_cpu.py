"""The host-only half of the cohort's outputs -- malva_amd/host/part_file.hpp and malva_amd/host/cohort_out.hpp: the PATH.part files, the
text of the --pairs and --sample-stats tables, the groups' count and packed-call streams, the two paste passes of the merged output --
checked by tools/cohort_out_host_check.cpp, a program of its own that needs no device.  It is built plain here (a sanitizer's runtime
would refuse to start where other libraries are preloaded); `make sanitize-host` builds the same program with -fsanitize."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cohort_out_host_check(tmp_path):
    exe = tmp_path / "cohort_out_host_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "malva_amd", "host"), "-o", str(exe),
                    os.path.join(ROOT, "tools", "cohort_out_host_check.cpp"), "-lz"], check=True, timeout=300)
    scratch = tmp_path / "scratch"
    scratch.mkdir()
    r = subprocess.run([str(exe), str(scratch)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", r.stdout + r.stderr
    assert r.stdout == "cohort_out_host_check: ok\n"
    assert not os.listdir(scratch)                                                # every file it made is gone again
