"""Builds one of the host kernel drivers (tests/*_host_driver.cpp on tests/host_kernel/) under AddressSanitizer + UBSan and runs it as
a stand-alone child process."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_driver(name, tmp_path):
    """the "case ..." lines of tests/<name>.cpp, after asserting a clean run: exit code 0, no sanitizer report, every case "ok" and
    "done fails=0" as the last line"""
    tests = os.path.join(ROOT, "tests")
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-pthread", "-Wno-attributes",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(tests, "host_kernel"),
                           "-I", os.path.join(ROOT, "snpmatch_amd", "csrc"), os.path.join(tests, name + ".cpp"), "-o", exe])
    # (a library the environment preloads may come before the ASan runtime: ASan copes as long as it does not replace malloc)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:verify_asan_link_order=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    lines = r.stdout.strip().split("\n")
    assert lines[-1] == "done fails=0"
    cases = [ln for ln in lines if ln.startswith("case ")]
    assert cases and all(ln.endswith(" ok") for ln in cases)
    return cases
