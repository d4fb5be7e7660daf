"""Reader of include/codetr_hip.h, the one written copy of the C ABI: its prototypes and integer #defines.

`functions`: name -> (return C type, [(C type, parameter name), ...]) in declaration order; `defines`: CODETR_<NAME> ->
int; `is_launch(name)`.  C types are spelled with single spaces ("const int64_t *").  The reader knows the header's own
vocabulary (`kind`) and raises HeaderError, naming the declaration, on anything else -- it never guesses.
"""
import os
import re

HEADER_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), "include",
                           "codetr_hip.h")
_SCALARS = {"int": "i", "int32_t": "i", "int64_t": "l", "uint32_t": "u", "float": "f"}
_DEFINE = re.compile(r"#\s*define\s+(CODETR_\w+)\s+\(?\s*(-?\d+)\s*\)?\s*$")
_DECL = re.compile(r"((?:const\s+)?\w+(?:\s*\*)?)\s*\b(\w+)\s*\((.*)\)", re.S)
_PARAM = re.compile(r"((?:\w+\s+)*\w+(?:\s*\*\s*(?:const\s+)?|\s+))(\w+)")


class HeaderError(ValueError):
    pass


def _spell(ctype):
    return " ".join(ctype.replace("*", " * ").split())


def kind(ctype, returned=False):
    """one letter per C type: p pointer, i int / int32_t, l int64_t, u uint32_t, f float; of a return type also v void
    and s `const char *`; None for a type the header does not use"""
    words = ctype.split()
    if words[-1] == "*":
        if returned:
            return "s" if words == ["const", "char", "*"] else None
        return None if "*" in words[:-1] or {"struct", "union", "enum"} & set(words) else "p"
    if returned and words == ["void"]:
        return "v"
    return _SCALARS.get(words[0]) if len(words) == 1 else None


def parse(text):
    """header text -> (functions, defines)"""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text).replace("\\\n", " ")
    defines, code = {}, []
    for line in text.splitlines():
        if line.lstrip().startswith("#"):
            m = _DEFINE.match(line.strip())
            if m:
                defines[m.group(1)] = int(m.group(2))
        else:
            code.append(line)
    code = re.sub(r'extern\s+"C"\s*\{', " ", "\n".join(code))
    functions = {}
    for decl in code.split(";"):
        decl = " ".join(decl.split())
        if decl in ("", "}"):   # (the closing brace of extern "C")
            continue
        m = _DECL.fullmatch(decl)
        if not m:
            raise HeaderError(f"cannot split the declaration `{decl}`")
        ret, name, params = _spell(m.group(1)), m.group(2), m.group(3).strip()
        if kind(ret, returned=True) is None:
            raise HeaderError(f"{name}: unknown return type `{ret}`")
        args = []
        for p in ([] if params == "void" else params.split(",")):
            pm = _PARAM.fullmatch(p.strip())
            if not pm or kind(_spell(pm.group(1))) is None:
                raise HeaderError(f"{name}: cannot read the parameter `{p.strip()}`")
            args.append((_spell(pm.group(1)), pm.group(2)))
        if name in functions:
            raise HeaderError(f"{name}: declared twice")
        functions[name] = (ret, args)
    return functions, defines


def is_launch(name):
    """a launch returns int and takes `void *stream` first; every other entry point is a host query"""
    ret, args = functions[name]
    return ret == "int" and args[:1] == [("void *", "stream")]


if not os.path.isfile(HEADER_PATH):
    raise ImportError(f"C ABI header not found at {HEADER_PATH}; the ctypes binding is derived from it, so the package "
                      "must run from a checkout that holds include/codetr_hip.h")
with open(HEADER_PATH) as _f:
    functions, defines = parse(_f.read())
