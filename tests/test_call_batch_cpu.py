"""The host-only slice around the device calls of `index` and `call` -- malva_amd/host/panel_batch.hpp (the flat arrays of general blocks
and lone records, which records a batch keeps and when it closes, the panel's genotype words) and malva_amd/host/call_text.hpp (the
per-sample lines, the merged output's lines and BCF records) -- checked by tools/call_batch_host_check.cpp, a program of its own that
needs no device.  It is built plain here; `make sanitize-host` builds the same program with -fsanitize=address,undefined."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_call_batch_host_check(tmp_path):
    exe = tmp_path / "call_batch_host_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "malva_amd", "host"), "-o", str(exe),
                    os.path.join(ROOT, "tools", "call_batch_host_check.cpp"), "-lz"], check=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", r.stdout + r.stderr
    assert r.stdout == "call_batch_host_check: ok\n"
