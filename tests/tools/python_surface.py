"""The public Python surface of the package as text: for every public name of playlist, library, song, decoder, the package
itself and of device.Context / device.Node, its signature and the sha256 of its docstring; for classes also their public
attributes.  Two trees have the same surface when the two dumps are equal (profiles/python_surface.txt).
  usage: python tests/tools/python_surface.py [ROOT]   (ROOT: the tree to read, default: this one)"""
import hashlib
import inspect
import os
import re
import sys

ROOT = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import bliss_rs_amd  # noqa: E402
from bliss_rs_amd import decoder, device, library, playlist, song  # noqa: E402


def doc_hash(obj):
    doc = inspect.getdoc(obj)
    return "-" if doc is None else hashlib.sha256(doc.encode()).hexdigest()[:16]


def sig(obj):
    try:
        return str(inspect.signature(obj))
    except (TypeError, ValueError):
        return "(no signature)"


def describe(owner, name, obj, out, depth=0):
    pad = "  " * depth
    if inspect.isclass(obj):
        out.append(f"{pad}{owner}.{name} class{sig(obj)} doc={doc_hash(obj)}")
        for attr, val in sorted(vars(obj).items()):
            if not attr.startswith("_"):
                describe(f"{owner}.{name}", attr, val, out, depth + 1)
    elif callable(obj) or isinstance(obj, (classmethod, staticmethod, property)):
        fn = obj.fget if isinstance(obj, property) else getattr(obj, "__func__", obj)
        out.append(f"{pad}{owner}.{name} {type(obj).__name__}{sig(fn)} doc={doc_hash(fn)}")
    elif not inspect.ismodule(obj):
        out.append(f"{pad}{owner}.{name} = {type(obj).__name__} {obj!r}"[:200])


def main():
    out = []
    for mod in (bliss_rs_amd, playlist, library, song, decoder):
        for name, obj in sorted(vars(mod).items()):
            if name.startswith("_") or inspect.ismodule(obj):
                continue
            if getattr(obj, "__module__", mod.__name__) not in (mod.__name__, None) and mod is not bliss_rs_amd:
                continue  # (a name imported from elsewhere is described where it lives)
            describe(mod.__name__, name, obj, out)
    for cls in (device.Context, device.Node):
        describe("bliss_rs_amd.device", cls.__name__, cls, out)
    text = "\n".join(out).replace(ROOT, "<root>")
    print(re.sub(r" at 0x[0-9a-f]+", "", text))  # (a default that is a function prints its address)


if __name__ == "__main__":
    main()
