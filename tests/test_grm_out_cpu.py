"""The host half of `call --cohort --grm` -- the text's rounding, the groups' word streams of malva_amd/host/cohort_out.hpp put side by side into
the cohort's bits, the chunked pass, GCTA's three files, the PATH.part hand-over -- checked by tools/grm_out_host_check.cpp, a program of its
own that needs no device: the definition's loop on the CPU (tools/grm_host_loop.cpp) stands in for it.  Four groupings of one cohort and chunk
sizes from one record to the whole table give the same bytes.  It is built plain here (a sanitizer's runtime would refuse to start where
other libraries are preloaded); `make sanitize-host` builds the same program with -fsanitize."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_grm_out_host_check(tmp_path):
    exe = tmp_path / "grm_out_host_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I" + os.path.join(ROOT, "malva_amd", "host"), "-o", str(exe),
                    os.path.join(ROOT, "tools", "grm_out_host_check.cpp"), "-lz"], check=True, timeout=300)
    scratch = tmp_path / "scratch"
    scratch.mkdir()
    r = subprocess.run([str(exe), str(scratch)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", r.stdout + r.stderr
    assert r.stdout == "grm_out_host_check: ok\n"
    assert not os.listdir(scratch)                                                # every file it made is gone again
