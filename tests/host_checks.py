"""What every *_host.py test of an operator asks besides its own questions, in one place: its entry points are in header, binding and
library at the ABI revision; a library without one of them is refused by name; a constant of its csrc/*_check.h; and its
tools/*_check.cpp, a stand-alone host program, built with ASan and UBSan and run as a child process.  Nothing here is loaded into
Python and nothing is preloaded."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, '3d-sdn_amd', 'csrc')
ABI = 20


def entry_points(names):
    """header, binding and library report revision 20, and every name is in exported_symbols(), in the library and declared
    `int NAME(` in the header.  -> the header's text with its wrapped comments joined (the history comment reads as one line)."""
    import sdn_hip
    src = open(os.path.join(ROOT, 'include', 'sdn_hip.h')).read()
    assert int(re.search(r'#define\s+SDN_ABI_VERSION\s+(\d+)', src).group(1)) == ABI == sdn_hip.ABI_VERSION == sdn_hip.lib().sdn_version()
    for name in names:
        assert name in sdn_hip.exported_symbols() and hasattr(sdn_hip.lib(), name), name
        assert re.search(r'\bint %s\(' % name, src), name
    return re.sub(r'\s*\n \*\s*', ' ', src)


def stale_library_is_refused(names):
    """a library that lacks one of `names` -- each withheld in turn -- was built before it was added: _declare says which and asks for
    a rebuild"""
    import sdn_hip
    for missing in names:
        class Stale:
            def __getattr__(self, name):
                if name == missing:
                    raise AttributeError(name)
                return getattr(sdn_hip.lib(), name)
        with pytest.raises(sdn_hip.SdnHipError, match='does not export %s -- rebuild' % missing):
            sdn_hip._declare(Stale())


def constexpr_int(header, name):
    """`constexpr int NAME = expr;` of csrc/<header>, expr a number or a constant expression of numbers"""
    text = open(os.path.join(CSRC, header)).read()
    return int(eval(re.search(r'constexpr int %s = ([^;]+);' % name, text).group(1), {}))


def run_check_program(name, headers, tmp_dir):
    """tools/<name>.cpp: a stand-alone program with its own main that includes only `headers` of csrc and no HIP; host code on the
    CPU in its own process, never loaded into Python.  Built with ASan and UBSan into tmp_dir and run once.  -> (return code, output)"""
    cxx = shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler'
    src = os.path.join(ROOT, 'tools', name + '.cpp')
    text = open(src).read()
    assert re.findall(r'#include "([^"]+)"', text) == list(headers) and 'int main()' in text and 'hip' not in text.lower()
    exe = str(tmp_dir / name)
    # the sanitizers' runtimes are linked into the program itself, so it runs the same whatever the environment preloads
    static = ['-static-libasan', '-static-libubsan'] if 'clang' not in os.path.basename(cxx) else ['-static-libsan']
    subprocess.check_call([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all'] + static +
                          ['-I' + CSRC, src, '-o', exe])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    print(run.stdout.decode())
    return run.returncode, run.stdout
