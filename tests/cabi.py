"""The one reading of the public headers (include/*.h) the C-ABI tests share: the functions a header declares, the value of a constant,
and what kind of ctypes type a parameter needs.  tests/test_cabi_headers.py holds every binding table to its header with these; the
feature tests take their header's declarations from here for what is specific to them."""
import os
import re

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
SCALARS = ("int", "int32_t", "uint32_t", "uint64_t", "size_t", "double")


def text(header):
    """the header without its comments"""
    hdr = open(os.path.join(INCLUDE, header)).read()
    return re.sub(r"//[^\n]*", " ", re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S))


def declarations(header):
    """[(return type, name, [parameter text, ...])] of the functions the header declares, in its order; (void) is no parameter"""
    out = []
    for ret, name, params in re.findall(r"([A-Za-z_][A-Za-z_0-9 ]*?[ *]+)(flg?_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", text(header)):
        params = [" ".join(p.split()) for p in params.split(",")]
        out.append((" ".join(ret.split()), name, [] if params == ["void"] else params))
    return out


def define(header, name):
    """the value text of `#define name value` or of the enumerator `name = value`"""
    m = re.search(r"^[ \t]*#[ \t]*define[ \t]+%s[ \t]+(\S[^\n]*?)[ \t]*$|\b%s[ \t]*=[ \t]*([^,}\n]+?)[ \t]*[,}\n]" % (name, name), text(header), re.M)
    if m is None:
        raise KeyError("%s has no %s" % (header, name))
    return m.group(1) or m.group(2)


def kind(param):
    """"pointer", or the scalar type word of a parameter; a scalar type that SCALARS does not list raises: add it there on purpose"""
    if "*" in param:
        return "pointer"
    words = [w for w in param.split()[:-1] if w != "const"]           # the last word is the parameter's name
    if len(words) != 1 or words[0] not in SCALARS:
        raise ValueError("parameter %r: no scalar type this module knows" % param)
    return words[0]
