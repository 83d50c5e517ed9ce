"""Builds the C++ check sources of tests/ (tests/*_check.cpp: the device headers compiled for the host) with one flag line."""
import os
import subprocess

TESTS = os.path.dirname(os.path.abspath(__file__))
FLAGS = ("-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-Wno-unknown-pragmas")


def build_check(name, out_dir, shared=True, flags=FLAGS, extra=()):
    """Compile tests/<name>.cpp into out_dir, as lib<name>.so (shared) or as the program <name>; returns the path of the result.
    flags: instead of FLAGS, for a check that is built another way on purpose; extra: on top of them (-D..., -fsanitize=...)."""
    out = os.path.join(str(out_dir), f"lib{name}.so" if shared else name)
    subprocess.check_call(["g++", *flags, *(("-fPIC", "-shared") if shared else ()), *extra, os.path.join(TESTS, name + ".cpp"), "-o", out])
    return out
