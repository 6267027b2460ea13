"""The planner's golden file (tests/golden/planner.json, written by tools/make_golden_planner.py): a JSON coding of the plain Python and
numpy objects a fingerprint and a plans dict hold that keeps their types -- int and ``np.int64`` are told apart, list and tuple, dict
and ``OrderedDict``, and a float goes through ``repr``, so it comes back bit for bit -- and the strict comparison of two such
objects.  Folder names inside the objects are stored relative to ``ROOT_MARK``."""
import json
import os
from collections import OrderedDict

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "planner.json")
ROOT_MARK = "@ROOT@"


def encode(obj, root=None):
    """``obj`` as JSON-able data; ``root``: a folder prefix that strings are stored without"""
    e = lambda o: encode(o, root)
    if isinstance(obj, str):
        return obj.replace(root, ROOT_MARK) if root else obj
    if isinstance(obj, np.bool_):
        return {"t": "np.bool_", "v": bool(obj)}
    if isinstance(obj, np.integer):
        return {"t": obj.dtype.name, "v": int(obj)}
    if isinstance(obj, np.floating):
        return {"t": obj.dtype.name, "v": float(obj)}
    if obj is None or isinstance(obj, (bool, int, float)):           # (behind the numpy scalars: np.float64 is a float)
        return obj
    if isinstance(obj, np.ndarray):
        assert obj.dtype.kind in "iufb", obj.dtype
        return {"t": "nd", "dtype": obj.dtype.str, "shape": list(obj.shape), "v": obj.ravel().tolist()}
    if isinstance(obj, list):
        return [e(o) for o in obj]
    if isinstance(obj, tuple):
        return {"t": "tuple", "v": [e(o) for o in obj]}
    if isinstance(obj, dict):
        assert type(obj) in (dict, OrderedDict), type(obj)
        return {"t": "odict" if isinstance(obj, OrderedDict) else "dict", "k": [e(k) for k in obj], "v": [e(v) for v in obj.values()]}
    raise TypeError("not a plain Python or numpy object: %r" % (type(obj),))


def decode(data, root=None):
    d = lambda o: decode(o, root)
    if isinstance(data, str):
        return data.replace(ROOT_MARK, root) if root else data
    if isinstance(data, list):
        return [d(o) for o in data]
    if not isinstance(data, dict):
        return data
    t = data["t"]
    if t == "nd":
        return np.array(data["v"], dtype=np.dtype(data["dtype"])).reshape(data["shape"])
    if t == "tuple":
        return tuple(d(o) for o in data["v"])
    if t in ("dict", "odict"):
        return (OrderedDict if t == "odict" else dict)((d(k), d(v)) for k, v in zip(data["k"], data["v"]))
    if t == "np.bool_":
        return np.bool_(data["v"])
    return np.dtype(t).type(data["v"])


def difference(a, b, where="plans"):
    """None when two objects hold the same keys, types and numbers, else a line that says where they first differ"""
    if type(a) is not type(b):
        return "%s: %r is a %s, %r a %s" % (where, a, type(a).__name__, b, type(b).__name__)
    if isinstance(a, dict):
        if list(a) != list(b):
            return "%s: keys %r and %r" % (where, list(a), list(b))
        for k in a:
            if type(k) is not type([x for x in b if x == k][0]):
                return "%s: key %r differs in type" % (where, k)
            d = difference(a[k], b[k], "%s[%r]" % (where, k))
            if d:
                return d
        return None
    if isinstance(a, (list, tuple)):
        if len(a) != len(b):
            return "%s: %d and %d entries" % (where, len(a), len(b))
        for i, (x, y) in enumerate(zip(a, b)):
            d = difference(x, y, "%s[%d]" % (where, i))
            if d:
                return d
        return None
    if isinstance(a, np.ndarray):
        if a.dtype != b.dtype or a.shape != b.shape or not np.array_equal(a, b):
            return "%s: %r and %r" % (where, a, b)
        return None
    return None if a == b else "%s: %r and %r" % (where, a, b)


def load():
    with open(GOLDEN) as f:
        return json.load(f)
