"""The C ABI of libmla_hip.so as ctypes, read from include/mla_hip.h: the header is the only statement of a signature.

build.sh force-includes the header into every translation unit, so the compiler rejects a declaration that disagrees with its
definition; this module turns the same declarations into restype / argtypes, so the Python side cannot disagree with them either.
Pure Python, no torch, no library load. A declaration it does not fully understand is a ValueError naming the function -- it never
guesses c_int or c_void_p, because ctypes would then truncate or misplace an argument without a word."""
import functools
import re
from ctypes import c_char_p, c_float, c_int, c_longlong, c_size_t, c_ulonglong, c_void_p

_SCALARS = {"int": c_int, "long long": c_longlong, "unsigned long long": c_ulonglong, "float": c_float, "size_t": c_size_t,
            "mla_stream_t": c_void_p}      # typedef struct ihipStream_t* mla_stream_t
_RETURNS = {"int": c_int, "long long": c_longlong, "const char*": c_char_p}
_DECL = re.compile(r"([\w\s*]+?)\b(mla_[a-z0-9_]+)\s*\(([^;]*)\)\s*;")
_NAME = re.compile(r"\b(mla_[a-z0-9_]+)\s*\(")          # every use of an entry point's name in front of a parenthesis


def _squeeze(s):
    return re.sub(r"\s*\*\s*", "*", " ".join(s.split()))


@functools.lru_cache(maxsize=None)      # ~1900 parameters, ~300 distinct spellings
def _argtype(p):
    if "..." in p or any(c in p for c in "()[]"):
        raise ValueError(f"parameter '{p}': variadic, array and function-pointer parameters have no ctypes mapping here")
    if "*" in p:
        return c_void_p
    words = [w for w in p.split() if w != "const"]
    for typ in (" ".join(words), " ".join(words[:-1])):         # unnamed parameter, then <type> <name>
        if typ in _SCALARS:
            return _SCALARS[typ]
    raise ValueError(f"parameter '{p}': type is none of {sorted(_SCALARS)} or a pointer")


def parse_header(text):
    """name -> (restype, [argtypes]) for every `<ret> mla_<name>(<params>);` of a header's text."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)
    table = {}
    for ret, fn, params in _DECL.findall(text):
        ret, params = _squeeze(ret), _squeeze(params)
        if fn in table:
            raise ValueError(f"{fn}: declared twice")
        if ret not in _RETURNS:
            raise ValueError(f"{fn}: return type '{ret}' is none of {sorted(_RETURNS)}")
        try:
            table[fn] = (_RETURNS[ret], [] if params in ("", "void") else [_argtype(p.strip()) for p in params.split(",")])
        except ValueError as e:
            raise ValueError(f"{fn}: {e}") from None
    skipped = set(_NAME.findall(text)) - set(table)
    if skipped:        # a spelling _DECL does not match must not drop out of the binding quietly
        raise ValueError(f"{sorted(skipped)}: named in front of '(' but not parsed as a declaration")
    return table


def load(path):
    """(restypes, signatures) of the header at `path`: name -> ctype and name -> list of ctypes."""
    try:
        with open(path) as f:
            text = f.read()
    except OSError as e:
        raise RuntimeError(f"{path} not readable ({e.strerror}): mla_amd derives the ctypes binding of libmla_hip.so from this header") from e
    try:
        table = parse_header(text)
    except ValueError as e:
        raise ValueError(f"{path}: {e}") from None
    return {k: v[0] for k, v in table.items()}, {k: v[1] for k, v in table.items()}
