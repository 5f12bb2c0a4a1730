"""The host decoder's call surface against tests/golden/decoder_api.json (tests/golden/make_decoder_api.py): every public name
of ``ViterbiDecoder``, ``DecodeStream`` and the module with its signature, the private names other code reaches for, docstrings,
and where ``DecodeStream`` lives.  Only imports the package: no GPU, no library."""
import inspect
import json
import os
import subprocess
import sys

import viterbi_spl_amd
from tests.golden import make_decoder_api as mk
from viterbi_spl_amd import decoder, stream

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASSES = {"ViterbiDecoder": decoder.ViterbiDecoder, "DecodeStream": decoder.DecodeStream}


def _golden():
    with open(mk.OUT) as fh:
        return json.load(fh)


def test_surface_equals_the_golden():
    want, got = _golden(), mk.surface()
    for name in CLASSES:
        assert sorted(got[name]["public"]) == sorted(want[name]["public"]), f"{name}: public names added or removed"
        for attr, sig in want[name]["public"].items():
            assert got[name]["public"][attr] == sig, (name, attr)
        assert got[name]["init"] == want[name]["init"], name
    assert got["module"] == want["module"]
    assert got == want
    assert (len(got["ViterbiDecoder"]["public"]), len(got["DecodeStream"]["public"])) == (45, 14)


def test_private_names_others_reach_for():
    want, got = _golden(), mk.surface()
    for name in CLASSES:
        assert sorted(want[name]["private_methods"]) == sorted(mk.PRIVATE_METHODS[name])
        assert got[name]["private_methods"] == want[name]["private_methods"], name
        assert sorted(want[name]["private_attributes"]) == sorted(mk.PRIVATE_ATTRIBUTES[name])
        assert all(got[name]["private_attributes"].values()), (name, got[name]["private_attributes"])
    assert inspect.ismodule(decoder._lib) and decoder._lib is viterbi_spl_amd._lib


def test_every_public_callable_has_a_docstring():
    for name, cls in CLASSES.items():
        assert (cls.__doc__ or "").strip(), name
        for attr, obj in mk.public_callables(cls):
            assert (inspect.getdoc(obj) or "").strip(), f"{name}.{attr} has no docstring"
    for fn in (decoder.decode, decoder.get_decoder):
        assert (inspect.getdoc(fn) or "").strip(), fn.__name__


def test_decode_stream_is_one_object():
    assert viterbi_spl_amd.DecodeStream is decoder.DecodeStream is stream.DecodeStream
    assert stream.DecodeStream.__module__ == "viterbi_spl_amd.stream"


def test_stream_module_imports_first():
    """A fresh interpreter whose first import of the package is the sessions' module."""
    r = subprocess.run([sys.executable, "-c", "import viterbi_spl_amd.stream as s; print(s.DecodeStream.__module__)"],
                       cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip() == "viterbi_spl_amd.stream"


def test_stream_module_does_not_import_the_decoder():
    """At import time ``stream.py`` binds nothing of ``decoder`` (the annotation is under TYPE_CHECKING)."""
    assert not hasattr(stream, "ViterbiDecoder") and not hasattr(stream, "decoder")
    src = inspect.getsource(stream)
    top_level = [ln for ln in src.splitlines() if ln.startswith(("import ", "from "))]
    assert not any("decoder" in ln for ln in top_level), top_level


def test_no_lazy_session_state():
    """Every attribute of a session is created in ``__init__``: nothing is looked up with a default."""
    for n, line in enumerate(inspect.getsource(stream).splitlines(), 1):
        assert "getattr(self" not in line, (n, line)
