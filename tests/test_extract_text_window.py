"""k_extract_text.h's XtWindow - the 16-byte register window a lane of k_xt_write assembles its run of
the output in - is plain C++: its text is cut out of the header, compiled with g++ under
AddressSanitizer and UBSan into a stand-alone program (tests/cpp/extract_window_test.cpp) and run
on the host over random runs, put sizes, skipped stretches, caps and alignments.  No GPU."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_extract_text_window_on_the_host(tmp_path):
    with open(os.path.join(ROOT, "one_amd", "csrc", "k_extract_text.h")) as f:
        found = re.search(r"struct XtWindow \{.*?\n\};\n", f.read(), re.S)
    assert found, "struct XtWindow not found in k_extract_text.h"
    (tmp_path / "xt_window.inc").write_text(found.group(0))
    prog = str(tmp_path / "extract_window_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize=alignment",
                    "-fno-sanitize-recover=all", "-I", str(tmp_path),
                    os.path.join(ROOT, "tests", "cpp", "extract_window_test.cpp"), "-o", prog],
                   check=True)
    assert subprocess.run([prog]).returncode == 2          # says so without its argument
    run = subprocess.run([prog, "30000"], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout == "window ok\n", run.stdout + run.stderr
