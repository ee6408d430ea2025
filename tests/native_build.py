"""Compiling the tests' native code (test infrastructure): a C file into a shared library that
ctypes loads, and a stand-alone checker program that is run as a child process.  The helpers
choose no flags: every caller passes its own, because they are part of what it tests (no
contraction and IEEE for the float references, warnings as errors and the sanitizers for the
checkers of host code)."""
import ctypes as C
import os
import subprocess


def shared_lib(src, out_dir, flags, libs=(), cc="gcc", timeout=None):
    """src compiled into out_dir as <name of src>.so, unless one at least as new as src is there,
    and loaded.  flags go before the source, libs ("-lm") after it."""
    so = os.path.join(str(out_dir), os.path.splitext(os.path.basename(str(src)))[0] + ".so")
    if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
        subprocess.run([cc, *flags, "-shared", "-fPIC", "-o", so, str(src), *libs], check=True, timeout=timeout)
    return C.CDLL(so)


def run_checker(tmp_path, sources, include_dirs, flags, cxx="g++", timeout=60):
    """The C++ sources compiled into one program under tmp_path (named after the first) and run
    without arguments under the time limit: status 0, or the assertion shows what it printed.
    Returns its stdout."""
    exe = str(tmp_path / os.path.splitext(os.path.basename(sources[0]))[0])
    includes = [a for d in include_dirs for a in ("-I", d)]
    subprocess.run([cxx, *flags, *includes, "-o", exe, *sources], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, f"{os.path.basename(exe)}: status {out.returncode}\n{out.stdout}{out.stderr}"
    return out.stdout
