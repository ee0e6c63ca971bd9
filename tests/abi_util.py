"""What the C-ABI tests share: the names the built library exports and the profiler's labels as the sources spell them."""
import os
import re
import shutil
import subprocess

import pytest

from sketchedit_amd import _lib


def exported_names(prefixes):
    """The unmangled names the built library defines that start with one of `prefixes` (a string or a tuple of them), as a set.
    Skips the calling test on a machine with neither nm nor llvm-nm."""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    nm = shutil.which("nm") or shutil.which("llvm-nm") or shutil.which("llvm-nm", path=os.path.join(rocm, "llvm", "bin"))
    if nm is None:
        pytest.skip("neither nm nor llvm-nm on this machine")
    out = subprocess.check_output([nm, "-D", "--defined-only", _lib.LIB_PATH], text=True)
    return {ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith(prefixes)}


def prof_labels():
    """(names, labels): the prof_label_name table of se_misc.hip and the enum ProfLabel of se_kernels.h, each in source order;
    the enum ends in PL_COUNT, which has no name"""
    misc = open(os.path.join(_lib.CSRC, "se_misc.hip")).read()
    enum = open(os.path.join(_lib.CSRC, "se_kernels.h")).read()
    names = re.findall(r'"(\w+)"', re.search(r"static const char\* n\[PL_COUNT\] = \{(.*?)\};", misc, re.S).group(1))
    labels = re.findall(r"PL_\w+", re.search(r"enum ProfLabel \{(.*?)\};", enum, re.S).group(1))
    return names, labels
