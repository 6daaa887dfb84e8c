"""The functions the public headers declare, found by a regular expression of its own (independent of the binding's parser)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_functions(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(hdsm_[a-z0-9_]+)\s*\(", txt)))
