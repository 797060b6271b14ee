"""Reader of the C ABI headers (include/afldm_hip.h, include/afldm_hip_experimental.h): the ctypes view of what they declare.

The headers are the one description of the boundary; _lib.py and _exp.py bind the libraries from what this module reads.  It
understands exactly the C subset the headers use - comments, `#define AFLDM_NAME <integer>`, anonymous enums with explicit
values, `typedef struct { ... } afldm_X;`, `typedef void* afldm_stream_t;` and `int | size_t | const char* afldm_f(params);` -
and raises HeaderError on anything else: nothing is guessed, nothing is skipped.  Needs neither torch nor a library."""
import ctypes
import os
import re

INCLUDE_DIR = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include"))

_SCALARS = {"int": ctypes.c_int, "float": ctypes.c_float, "size_t": ctypes.c_size_t, "long long": ctypes.c_longlong,
            "unsigned int": ctypes.c_uint}
_POINTEES = set(_SCALARS) | {"void", "char", "unsigned char"}       # what a plain (c_void_p) pointer may point to
_RESTYPES = (ctypes.c_int, ctypes.c_size_t, ctypes.c_char_p)

_SKIP = re.compile(r'extern\s+"C"\s*\{|\}')                          # the __cplusplus wrapper (its #ifdef lines are gone by then)
_STRUCT = re.compile(r"typedef\s+struct\s*\{([^{}]*)\}\s*(\w+)\s*;")
_ENUM = re.compile(r"enum\s*\{([^{}]*)\}\s*;")
_TYPEDEF = re.compile(r"typedef\s+([^;{}()]+?)(\w+)\s*;")
_FUNCTION = re.compile(r"([^;{}()]+?)\b(\w+)\s*\(([^;{}()]*)\)\s*;")
_DEFINE = re.compile(r"#\s*define\s+(\w+)(?:\s+(.*?))?\s*$")
_INT = re.compile(r"[-+]?\d+$")
_SPACE = re.compile(r"\s*")


class HeaderError(ValueError):
    pass


class Abi:
    """What one header declares: functions {name: (argtypes, restype)}, structs {C name: ctypes.Structure class}, typedefs
    {name: ctypes type} and constants {name: int}, each in header order.  `base` is the Abi of a header it includes."""

    def __init__(self, text, base=None, where="<header>"):
        self.where = where
        self.functions, self.constants = {}, {}
        self.structs = dict(base.structs) if base else {}
        self.typedefs = dict(base.typedefs) if base else {}
        self._ctypes = {}
        self._parse(text)

    def ctype(self, decl, what):
        """The ctypes type of the C type `decl` (the table in INTEGRATION.md); `what` names the declaration in the error."""
        if decl not in self._ctypes:                     # a header spells a few dozen types a thousand times
            self._ctypes[decl] = self._ctype(decl, what)
        return self._ctypes[decl]

    def _ctype(self, decl, what):
        words = re.sub(r"\bconst\b", " ", decl).replace("*", " * ").split()
        stars = words.count("*")
        base = " ".join(w for w in words if w != "*")
        if stars == 0 and base in _SCALARS:
            return _SCALARS[base]
        if stars == 0 and base in self.typedefs:
            return self.typedefs[base]
        if stars == 1 and base == "char":
            return ctypes.c_char_p
        if stars == 1 and base in self.structs:
            return ctypes.POINTER(self.structs[base])
        if stars >= 1 and (base in _POINTEES or base in self.typedefs):
            return ctypes.c_void_p
        raise HeaderError(f"{self.where}: {what}: unknown type '{' '.join(decl.split())}'")

    def _declarator(self, text, what):
        text = " ".join(text.split())
        cut = max(text.rfind(" "), text.rfind("*")) + 1  # the name is the last word
        if not cut or not text[cut:].isidentifier():
            raise HeaderError(f"{self.where}: {what}: cannot read '{text}' as a type and a name")
        return text[:cut], text[cut:]

    def _struct(self, body, name):
        fields = []
        for decl in body.split(";"):
            if not decl.strip():
                continue
            first, *more = decl.split(",")               # `int C1, C2;` names several fields of one type
            ctype_text, field = self._declarator(first, f"struct {name}")
            t = self.ctype(ctype_text, f"struct {name}, field {field}")
            for extra in [field] + [e.strip() for e in more]:
                if not re.fullmatch(r"[A-Za-z_]\w*", extra):
                    raise HeaderError(f"{self.where}: struct {name}: cannot read the declarator '{extra}'")
                fields.append((extra, t))
        py_name = "".join(w.capitalize() for w in name.replace("afldm_", "", 1).split("_"))
        self.structs[name] = type(py_name, (ctypes.Structure,), {"_fields_": fields, "__doc__": f"{name} ({self.where})"})

    def _enum(self, body):
        for item in body.split(","):
            m = re.fullmatch(r"\s*(\w+)\s*=\s*([-+]?\d+)\s*", item)
            if not m:
                raise HeaderError(f"{self.where}: enum entry '{item.strip()}' is not NAME = <integer>")
            self.constants[m.group(1)] = int(m.group(2))

    def _function(self, ret, name, params):
        restype = self.ctype(ret, f"{name}, return type")
        if restype not in _RESTYPES:
            raise HeaderError(f"{self.where}: {name}, return type: unknown type '{' '.join(ret.split())}'")
        argtypes = []
        if params.strip() != "void":
            for p in params.split(","):
                ctype_text, pname = self._declarator(p, name)
                argtypes.append(self.ctype(ctype_text, f"{name}, parameter {pname}"))
        self.functions[name] = (argtypes, restype)

    def _parse(self, text):
        text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
        text = re.sub(r"//[^\n]*", " ", text)
        code = []
        for line in text.splitlines():
            if not line.lstrip().startswith("#"):
                code.append(line)
                continue
            m = _DEFINE.match(line.strip())
            if m and m.group(2):                          # `#define GUARD` and #if / #include / #endif carry no value
                if not _INT.match(m.group(2)):
                    raise HeaderError(f"{self.where}: #define {m.group(1)} {m.group(2)} is not an integer")
                self.constants[m.group(1)] = int(m.group(2))
        text, pos = "\n".join(code), 0
        while True:
            pos = _SPACE.match(text, pos).end()
            if pos == len(text):
                return
            for pattern in (_SKIP, _STRUCT, _ENUM, _TYPEDEF, _FUNCTION):
                m = pattern.match(text, pos)
                if m:
                    break
            else:
                raise HeaderError(f"{self.where}: cannot read the declaration at '{' '.join(text[pos:pos + 80].split())}'")
            if pattern is _STRUCT:
                self._struct(m.group(1), m.group(2))
            elif pattern is _ENUM:
                self._enum(m.group(1))
            elif pattern is _TYPEDEF:
                self.typedefs[m.group(2)] = self.ctype(m.group(1), f"typedef {m.group(2)}")
            elif pattern is _FUNCTION:
                self._function(*m.groups())
            pos = m.end()

    def names(self, prefix):
        """{lower-cased suffix: value} of the constants whose names start with `prefix`, ordered by value."""
        found = {n[len(prefix):].lower(): v for n, v in self.constants.items() if n.startswith(prefix)}
        return dict(sorted(found.items(), key=lambda kv: kv[1]))

    def bind(self, lib):
        """Set argtypes / restype of every declared function on the loaded library; a symbol the library lacks is an
        AttributeError.  Returns the sorted names."""
        for name, (argtypes, restype) in self.functions.items():
            fn = getattr(lib, name)
            fn.argtypes, fn.restype = argtypes, restype
        return sorted(self.functions)


def read(filename, base=None):
    path = os.path.join(INCLUDE_DIR, filename)
    if not os.path.exists(path):
        raise ImportError(f"{path} is missing: the ctypes bindings of afldm_amd are read from the C headers")
    with open(path) as f:
        return Abi(f.read(), base, where=f"include/{filename}")
