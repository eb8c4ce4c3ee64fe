"""Host model of the match kernel's serial link (tools/micro/chain_link_model.cpp:
whole groups without bounds selects, the ragged rest as before, the progress
word behind the link stores) built with ASan + UBSan as a stand-alone program
and run on the CPU: every variant gives the plain definition's links."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(not shutil.which("g++"), reason="g++ missing")
def test_chain_link_model_sanitized(tmp_path):
    exe = str(tmp_path / "chain_link_model")
    b = subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-o", exe, os.path.join(ROOT, "tools", "micro", "chain_link_model.cpp")],
                       capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    assert p.stdout.strip().endswith("chain_link_model ok")
    assert "residues missed 0" in p.stdout
