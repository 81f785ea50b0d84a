"""What include/slu_hip.h declares, read with plain `re` for the tests: the entry point names and how many arguments each
takes.  It imports nothing of slu_hip on purpose — slu_hip/lib.py derives its binding table from the same file with its own
parser, and the tests hold the two readers against each other."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "slu_hip.h")


def header_text():
    with open(HEADER) as f:
        return f.read()


def code(text=None):
    """The header without its comments."""
    text = header_text() if text is None else text
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


def header_functions(text=None):
    """Sorted names of everything that looks like an entry point: `slu_name(` outside a block comment."""
    text = header_text() if text is None else text
    return sorted(set(re.findall(r"\b(slu_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S))))


def arg_counts(text=None):
    """name -> number of parameters, by counting the commas between a declaration's parentheses ((void): 0)."""
    counts = {}
    for name, params in re.findall(r"\b(slu_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", code(text)):
        assert name not in counts, name
        counts[name] = 0 if params.strip() == "void" else len(params.split(","))
    return counts


def abi_version(text=None):
    return int(re.search(r"#define\s+SLU_ABI_VERSION\s+(\d+)", header_text() if text is None else text).group(1))
