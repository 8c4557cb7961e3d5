"""The command line of malva-geno -- malva_amd/host/options.hpp (one table of options, one parser) and usage.hpp -- checked by
tools/options_host_check.cpp: a program of its own that runs a list of command lines through parse_arguments and compares, record by
record, with tests/golden/options_cases.jsonl.  That file and tests/golden/usage.txt were recorded from the parser as it stood in
main.cpp before it became a table (the same program built against it): they say what the command line has always done.  The check is
built plain here; `make sanitize-host` builds it with -fsanitize=address,undefined."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin", "malva-geno")
GOLDEN = os.path.join(ROOT, "tests", "golden")

needs_cli = pytest.mark.skipif(not os.path.exists(BIN), reason="bin/malva-geno not built")


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = tmp_path_factory.mktemp("options") / "options_host_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "malva_amd", "host"), "-o", str(exe),
                    os.path.join(ROOT, "tools", "options_host_check.cpp")], check=True, timeout=300)
    return str(exe)


def _usage():
    with open(os.path.join(GOLDEN, "usage.txt"), newline="") as f:
        return f.read()


def test_options_host_check(check):
    r = subprocess.run([check, os.path.join(GOLDEN, "options_cases.jsonl")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", r.stdout + r.stderr
    assert r.stdout == "options_host_check: ok\n"


def test_usage_text_is_the_recorded_one(check):
    r = subprocess.run([check, "--usage"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stderr == ""
    assert r.stdout == _usage()


@needs_cli
def test_help_prints_the_usage_to_stdout():
    for cmd in ("call", "index"):
        for flag in ("-h", "--help"):
            r = subprocess.run([BIN, cmd, flag], capture_output=True, text=True, timeout=60)
            assert r.returncode == 0 and r.stderr == "", (cmd, flag, r.stderr)
            assert r.stdout == _usage()


@needs_cli
def test_messages_ahead_of_help_come_first():
    r = subprocess.run([BIN, "call", "--ld-window", "0", "-h", "a", "b", "c"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    assert r.stderr == "malva : --ld-window takes a whole number 1..1024\n"
    assert r.stdout == _usage()
