#!/usr/bin/env python3
"""Record the host decoder's call surface (tests/golden/decoder_api.json, compared exactly by tests/test_decoder_api_host.py):
every public attribute of ``ViterbiDecoder`` and ``DecodeStream`` and the module-level ``decode`` / ``get_decoder`` with its
signature, plus the private names other code reaches for (bench.py, reference_api.py, the scripts and the tests).

Only imports the package and uses ``inspect``: no GPU, no library.  Run it only where the surface is MEANT to change; a refactor
of the host layer must reproduce the file byte for byte.

    python tests/golden/make_decoder_api.py [output.json]
"""
import inspect
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
OUT = os.path.join(HERE, "decoder_api.json")

CONSTANTS = ("COUNTERS", "FAMILIES", "MAX_LOOKBACK")
# private names with users outside the class: methods (signature pinned) and the attributes ``__init__`` creates
PRIVATE_METHODS = {"ViterbiDecoder": ("_workspace", "_call_workspace", "_obs_struct", "_greedy_groups", "_plan_segments"),
                   "DecodeStream": ("_handle",)}
PRIVATE_ATTRIBUTES = {"ViterbiDecoder": ("_plan", "_ws", "_ws_slots", "_options"), "DecodeStream": ()}


def describe(cls, name):
    """What the golden file says about attribute `name` of `cls`: "property", the repr of a constant, or the signature."""
    raw = inspect.getattr_static(cls, name)
    if isinstance(raw, property):
        return "property"
    if name in CONSTANTS:
        return repr(raw)
    kind = "staticmethod " if isinstance(raw, staticmethod) else ""
    return kind + str(inspect.signature(getattr(cls, name)))


def public_callables(cls):
    """(name, object) of every public method, static method and property of `cls`."""
    for name in sorted(vars(cls)):
        if not name.startswith("_") and name not in CONSTANTS:
            raw = inspect.getattr_static(cls, name)
            yield name, raw.fget if isinstance(raw, property) else getattr(cls, name)


def init_attributes(cls):
    """The names ``cls.__init__`` stores on ``self`` (the attribute names of its code object that appear as ``self.<name> =``)."""
    src = inspect.getsource(cls.__init__)
    return sorted(n for n in cls.__init__.__code__.co_names if f"self.{n} =" in src or f"self.{n}:" in src)


def surface():
    import viterbi_spl_amd
    from viterbi_spl_amd import decoder
    rec = {"module": {n: str(inspect.signature(getattr(decoder, n))) for n in ("decode", "get_decoder")}}
    for cls in (decoder.ViterbiDecoder, decoder.DecodeStream):
        name = cls.__name__
        assert getattr(viterbi_spl_amd, name) is cls
        rec[name] = {"init": str(inspect.signature(cls.__init__)),
                     "public": {n: describe(cls, n) for n in sorted(vars(cls)) if not n.startswith("_")},
                     "private_methods": {n: describe(cls, n) for n in PRIVATE_METHODS[name]},
                     "private_attributes": {n: n in init_attributes(cls) for n in PRIVATE_ATTRIBUTES[name]}}
    rec["module"]["_lib"] = type(decoder._lib).__name__
    return rec


if __name__ == "__main__":
    rec = surface()
    out = sys.argv[1] if len(sys.argv) > 1 else OUT
    with open(out, "w") as fh:
        json.dump(rec, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(f"{out}: " + ", ".join(f"{len(rec[c]['public'])} public names on {c}" for c in ("ViterbiDecoder", "DecodeStream")))
