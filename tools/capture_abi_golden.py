"""Golden of the ctypes binding of libmla_hip.so: what every exported function carries after hip.lib() -- needs the built library, no GPU.

    PYTHONDONTWRITEBYTECODE=1 python tools/capture_abi_golden.py

Reads restype and argtypes off the loaded library's function objects, so it records the binding in force whatever built it: the
committed tests/golden/abi_signatures.json was captured on the last commit whose tables were written by hand (the _SIGNATURES literal,
the two register_signatures blocks, the restype fix-ups and the two c_char_p functions in lib()), before mla_amd/hip.py started to
derive them from include/mla_hip.h. tests/test_abi.py holds the derived binding to it. Re-run only when the header changes on purpose,
and read the diff of the JSON: it is the ABI change.
Writes {symbol: {"restype": ctype name, "argtypes": [ctype names]}} sorted by symbol, one symbol per line. The names are the classes'
own __name__ on 64-bit Linux, where ctypes makes c_longlong an alias of c_long and c_size_t / c_ulonglong aliases of c_ulong."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mla_amd import hip  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "abi_signatures.json")


def main():
    lib = hip.lib()
    table = {}
    for name in hip.exported_symbols():
        fn = getattr(lib, name)
        table[name] = {"restype": fn.restype.__name__, "argtypes": [t.__name__ for t in fn.argtypes]}
    rows = [f"  {json.dumps(k)}: {json.dumps(v)}" for k, v in sorted(table.items())]
    with open(OUT, "w") as f:
        f.write("{\n" + ",\n".join(rows) + "\n}\n")
    print(f"abi_signatures.json: {len(table)} symbols, restypes {sorted({v['restype'] for v in table.values()})}")


if __name__ == "__main__":
    main()
