"""Result egress parity: TableInfo::print / printall of include/aquery against the text the REFERENCE's own printer
produced for the same tables (tests/golden/print_shapes.txt, the stdout of oracle/_ref/print_shapes_ref = oracle/ref_harness.cpp
compiled with the reference headers over tests/emitted/print_shapes.inc).  Host-only: runs without a GPU."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
EM = os.path.join(HERE, "emitted")


def test_print_and_printall_text_is_the_reference_text_byte_for_byte():
    subprocess.check_call(["make", "-C", EM, "build/print_shapes"], stdout=subprocess.DEVNULL)
    out = subprocess.run([os.path.join(EM, "build", "print_shapes")], capture_output=True, timeout=120)
    assert out.returncode == 0, out.stderr.decode()
    want = open(os.path.join(HERE, "golden", "print_shapes.txt"), "rb").read()
    assert out.stdout == want
    assert want.count(b"-- ") == 10 and b"1180591620717411303429" in want and b"133.333333" in want


def test_golden_text_is_what_the_reference_prints(ref_answers):
    """the golden text is the reference printer's own output: its digest was recorded from oracle/_ref/print_shapes_ref, which is
    run again where it is built"""
    ref_exe = os.path.join(os.path.dirname(HERE), "oracle", "_ref", "print_shapes_ref")
    want = open(os.path.join(HERE, "golden", "print_shapes.txt"), "rb").read()
    ref_answers.check("egress/print_shapes", want, lambda r: subprocess.run([ref_exe], capture_output=True, timeout=120, check=True).stdout)
