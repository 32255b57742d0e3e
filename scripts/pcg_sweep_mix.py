#!/usr/bin/env python3
"""Prints the reference table of the PCG sweep kernels (tests/test_cpu_pcg_window_kernel_resources.py: SWEEP_PARENT) for a source tree:
per arithmetic flavour and mangled name the digest of the sorted (mnemonic, count) list, the number of instructions, NumVgprs,
ScratchSize and Occupancy, compiled with that tree's Makefile flags through the helpers of tests/test_cpu_kernel_resources.py.
usage: pcg_sweep_mix.py [root of the tree to compile, default: this one]     e.g. a `git worktree add --detach <dir> <commit>`"""
import os
import pathlib
import re
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tests.test_cpu_kernel_resources as kr   # noqa: E402
from tests.isa_pins import _functions, _histogram   # noqa: E402

SWEEP = re.compile(r"\d+pcg_(window_)?(init|step1|step1_lds)_kernelI")

tree = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else ROOT
kr.CSRC, kr.ROOT = os.path.join(tree, "badslam_amd", "csrc"), tree     # what _compile reads the sources and the C ABI header from
with tempfile.TemporaryDirectory() as d:
    print("SWEEP_PARENT = {")
    for flavour in ("exact", "fast"):
        print(f'    "{flavour}": {{')
        for unit in ("kernels_pcg", "kernels_pcg_window"):
            listing = kr._compile(pathlib.Path(d), unit, kr._fast_flags(unit) if flavour == "fast" else [], "_" + flavour)
            functions, kernels = _functions(listing), kr._kernels(listing)
            for name in sorted(n for n in functions if SWEEP.search(n)):
                mix, total = _histogram(functions[name])
                print(f'        "{name}":\n            ("{mix}", {total}, {kernels[name][1]}, {kernels[name][2]}, {kernels[name][3]}),')
        print("    },")
    print("}")
