"""The cached Sokoban turn's host-checkable pieces (ragen_amd/csrc/lean_turn.hpp and board_step.hpp's
valid_slots), built with g++ (tests/native/lean_turn_driver.cpp): the compile-time-K action fetch
-- the dword offsets it addresses and the bytes it assembles -- against a byte-wise restatement for
K = 1..8, every byte shift, every base misalignment and random dwords, with the addressed dwords
held to load_actions_at's (never outside the dwords that hold the row); and the shared valid-byte
helper against board_step.hpp's own valid_bytes over the 64-bit slot range."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_action_fetch_and_valid_slots_match_restatement(tmp_path):
    exe = str(tmp_path / "lean_turn_driver")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), "-I",
                    os.path.join(ROOT, "ragen_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "lean_turn_driver.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout + r.stderr
    assert int(r.stdout.split()[1]) > 500000
