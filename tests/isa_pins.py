"""What the build-time pins of the kernel-resource tests take from a hipcc -S listing of gfx950 code (a plain helper module: the tests
that pin code import these names, tests/test_cpu_pcg_window_kernel_resources.py re-exports the first two)."""
import collections
import hashlib
import re


def _functions(listing):
    """mangled name -> the function's whole code, from its label to its .Lfunc_end label (every exit included)"""
    return {m.group(1): m.group(2) for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", listing, re.S | re.M)}


def _digest(body):
    body = re.sub(r";.*", "", body)                          # comments
    body = re.sub(r"\.L(BB|tmp)\d+_", r".L\1_", body)        # label numbers follow the function's place in the unit
    return hashlib.sha256("\n".join(line.rstrip() for line in body.splitlines() if line.strip()).encode()).hexdigest()[:24]


def _histogram(body):
    """(digest of the sorted (mnemonic, count) list, number of instructions) of a function's code: what survives a change of register
    numbering or instruction order (the counting of scripts/isa_histogram.py, up to the function's end)"""
    hist = collections.Counter(line.split()[0] for line in body.splitlines()
                               if line.startswith("\t") and not line.strip().startswith((".", ";")))
    mix = ",".join(f"{mnemonic}:{count}" for mnemonic, count in sorted(hist.items()))
    return hashlib.sha256(mix.encode()).hexdigest()[:16], sum(hist.values())
