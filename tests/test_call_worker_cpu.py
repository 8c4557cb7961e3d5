"""What one batch of `call` does on the device, and the pipeline that keeps as many batches in flight as there are devices --
malva_amd/host/call_worker.hpp and malva_amd/host/device.hpp -- checked by tools/call_worker_host_check.cpp: a program of its own that
defines every mg_* entry point the worker calls and is linked without libmalva_hip, so it needs no device.  It is built plain here;
`make sanitize-host` builds the same program with -fsanitize=address,undefined and again with -fsanitize=thread."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_call_worker_host_check(tmp_path):
    exe = tmp_path / "call_worker_host_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-pthread", "-I" + os.path.join(ROOT, "malva_amd", "host"), "-o", str(exe),
                    os.path.join(ROOT, "tools", "call_worker_host_check.cpp"), "-lz"], check=True, timeout=300)
    r = subprocess.run([str(exe), str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", r.stdout + r.stderr
    assert r.stdout == "call_worker_host_check: ok\n"
    assert sorted(os.listdir(tmp_path)) == ["call_worker_host_check"]  # (its scratch files are gone)
