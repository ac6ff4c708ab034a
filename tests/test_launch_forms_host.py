"""Device-free tests of bliss-rs_amd/csrc/launch_forms.hpp, the launch scaffolding every scan family shares: the (d, metric,
diagonal-M) ladder, the device-fill policy and the label sort's workspace words, as a stand-alone program (plain and under
sanitizers), and that the header stays free of HIP."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_launch_forms.cpp")
HPP = os.path.join(ROOT, "bliss-rs_amd", "csrc", "launch_forms.hpp")
SAN_CXX = "/opt/rocm/lib/llvm/bin/clang++"


def _check_program(exe, env=None):
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 0, (out.stdout[-500:], out.stderr[-3000:])
    assert "Sanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-3000:]
    assert out.stdout.strip() == "launch_forms ok"


def test_launch_forms_header(tmp_path):
    exe = tmp_path / "test_launch_forms"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", SRC, "-o", str(exe)])
    _check_program(exe)


@pytest.mark.skipif(not os.path.exists(SAN_CXX), reason="needs the ROCm clang for -fsanitize=address,undefined")
def test_launch_forms_header_under_address_and_ub_sanitizer(tmp_path):
    """the same stand-alone program built with -fsanitize=address,undefined: exit 0, no report"""
    exe = tmp_path / "test_launch_forms_san"
    subprocess.check_call([SAN_CXX, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", SRC,
                           "-o", str(exe)])
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1 exitcode=66", UBSAN_OPTIONS="halt_on_error=1 print_stacktrace=1")
    _check_program(exe, env)


def test_launch_forms_header_is_device_free():
    code = re.sub(r"//[^\n]*", "", open(HPP).read())
    assert "hip" not in code.lower() and "__device__" not in code and "__global__" not in code
    assert re.findall(r"#include\s+[<\"]([^>\"]+)", code) == ["stddef.h", "stdint.h", "type_traits"]
    # the metric ids have one home: the arithmetic header takes them from here
    math = open(os.path.join(ROOT, "bliss-rs_amd", "csrc", "pairwise_math.hpp")).read()
    assert '#include "launch_forms.hpp"' in math and "METRIC_EUCLIDEAN =" not in math

