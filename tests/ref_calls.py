"""The reference's answers, recorded: lets tests/test_oracle_vs_ref.py pin the oracle against the reference where the
reference is not at hand.

`Reference(Record(name, live))` stands in for the module oracle.ref.module() -- the reference's own sources compiled into
oracle/_ref, behind the oracle's API.  Every call made through it (module functions, constructors, methods of the objects
they return) is one entry of the record: its name, a SHA-256 of its arguments and the reference's answer.  Each call is
also made on a shadow, the oracle (oracle.oracle, the same API); an array of the answer that is bit-identical to the
shadow's is stored as its digest, any other one in full, so the record stays small.
  * oracle/_ref is available (`live`): the calls go to the reference.  LT_REF_RECORD=1 writes the record to
    tests/golden/ref_calls/<name>.npz, with the hash of the tree oracle/_ref was built against; otherwise the live answers
    must be the committed ones, so a stale record fails where the reference exists.
  * oracle/_ref is not available: the answers come from the record, call by call.  A call whose name or arguments differ
    from the recorded one fails (the test changed: record again where the reference exists); a digest-stored array is the
    shadow's array once its digest is the recorded one, and fails otherwise (the oracle no longer computes the reference's
    bits).
Either way the test then compares the oracle's answers with the reference's by its own assertions."""
import builtins
import hashlib
import json
import os

import numpy as np

RECORD_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_calls")



class _Handle:
    """An object the reference returned (a triangulator, a track set): its methods are calls of the record too."""

    def __init__(self, rec, oid):
        self._rec, self._oid = rec, oid

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)
        return lambda *a, **k: self._rec.call(self._oid, name, a, k)


def _digest_into(h, x):
    if isinstance(x, _Handle):
        h.update(b"H%d;" % x._oid)
    elif isinstance(x, (np.ndarray, np.generic)):
        a = np.ascontiguousarray(x)
        h.update(b"A" + str(a.dtype).encode() + str(a.shape).encode() + a.tobytes())
    elif isinstance(x, dict):
        h.update(b"D%d{" % len(x))
        for k in sorted(x, key=str):
            _digest_into(h, k)
            _digest_into(h, x[k])
        h.update(b"}")
    elif isinstance(x, (list, tuple)):
        h.update(b"L%d[" % len(x))
        for v in x:
            _digest_into(h, v)
        h.update(b"]")
    else:
        h.update(b"S" + repr(x).encode() + b";")


def _digest(*xs):
    h = hashlib.sha256()
    for x in xs:
        _digest_into(h, x)
    return h.hexdigest()[:32]


def _is_data(v):
    return v is None or isinstance(v, (bool, int, float, str, np.ndarray, np.generic, tuple, list, dict))


class Record:
    def __init__(self, name, live_module=None, shadow_module=None):
        from oracle import oracle as shadow
        self.name, self.path = name, os.path.join(RECORD_DIR, name + ".npz")
        self.live, self.shadow = live_module, shadow_module or shadow
        self.recording = live_module is not None and os.environ.get("LT_REF_RECORD") == "1"
        self.entries, self.arrays = [], {}
        self.objects = {0: (live_module, self.shadow)}   # oid -> (reference object or None, shadow object)
        self.saved = None
        if not self.recording:
            self._load()

    # -- storage ------------------------------------------------------------------------------------------------
    def _load(self):
        if not os.path.exists(self.path):
            assert self.live is not None, (f"no recorded reference answers {os.path.relpath(self.path)}: record them where "
                                           "oracle/_ref can be built (LT_REF_RECORD=1)")
            return
        with np.load(self.path) as z:
            meta = json.loads(bytes(z["__meta__"]).decode())
            self.saved = dict(meta, arrays={k: z[k] for k in z.files if k != "__meta__"})

    def save(self, tree_hash):
        os.makedirs(RECORD_DIR, exist_ok=True)
        meta = json.dumps({"tree_source_hash": tree_hash, "entries": self.entries}, separators=(",", ":")).encode()
        np.savez_compressed(self.path, __meta__=np.frombuffer(meta, np.uint8), **self.arrays)

    # -- the reference's answer <-> JSON + arrays (the shadow's answer alongside) -------------------------------
    def _enc(self, v, sh):
        if v is None or isinstance(v, (bool, str)):
            return v
        if isinstance(v, float):
            return {"f": repr(v)}
        if isinstance(v, int):
            return v
        if isinstance(v, (np.ndarray, np.generic)):
            a, s = np.asarray(v), (np.asarray(sh) if isinstance(sh, (np.ndarray, np.generic)) else None)
            e = {"scalar": isinstance(v, np.generic)}
            if s is not None and s.dtype == a.dtype and s.shape == a.shape \
                    and s.tobytes() == a.tobytes():
                e["h"] = _digest(a)
            else:
                e["a"] = "a%d" % len(self.arrays)
                self.arrays[e["a"]] = a
            return e
        if isinstance(v, (tuple, list)):
            sh = sh if isinstance(sh, (tuple, list)) and len(sh) == len(v) else [None] * len(v)
            return {"t" if isinstance(v, tuple) else "l": [self._enc(x, y) for x, y in zip(v, sh)]}
        if isinstance(v, dict):
            sh = sh if isinstance(sh, dict) else {}
            return {"d": [[k, self._enc(x, sh.get(k))] for k, x in v.items()]}
        raise TypeError(f"{self.name}: cannot record an answer of type {type(v).__name__}")

    def _dec(self, e, sh, arrays, where):
        if not isinstance(e, dict):
            return e
        if "o" in e:
            return ("object", e["o"])
        if "f" in e:
            return float(e["f"])
        if "a" in e or "h" in e:
            if "a" in e:
                a = arrays[e["a"]]
            else:
                a = np.asarray(sh) if isinstance(sh, (np.ndarray, np.generic)) else None
                assert a is not None and _digest(a) == e["h"], (
                    f"{where}: the oracle's answer is not the reference's recorded one (digest differs)")
            return a[()] if e["scalar"] else a
        if "t" in e or "l" in e:
            xs = e.get("t", e.get("l"))
            sh = sh if isinstance(sh, (tuple, list)) and len(sh) == len(xs) else [None] * len(xs)
            out = [self._dec(x, y, arrays, where) for x, y in zip(xs, sh)]
            return tuple(out) if "t" in e else out
        if "d" in e:
            sh = sh if isinstance(sh, dict) else {}
            return {k: self._dec(x, sh.get(k), arrays, where) for k, x in e["d"]}
        raise AssertionError(f"{where}: unreadable record entry {e}")

    # -- one call -----------------------------------------------------------------------------------------------
    def call(self, oid, name, args, kwargs):
        n = len(self.entries)
        where = f"{self.name}: call {n} ({name})"
        entry = {"call": [oid, name], "args": _digest(list(args), dict(kwargs))}
        self.entries.append(entry)

        def unwrap(side):
            return [self.objects[a._oid][side] if isinstance(a, _Handle) else a for a in args]
        sh_ret = None
        try:
            sh_ret = getattr(self.objects[oid][1], name)(*unwrap(1), **kwargs)
        except Exception:   # (the reference's answer decides: recorded, or compared digest by digest)
            pass
        if self.live is not None:
            try:
                ret = getattr(self.objects[oid][0], name)(*unwrap(0), **kwargs)
            except Exception as ex:
                entry.update({"raise": type(ex).__name__ if hasattr(builtins, type(ex).__name__) else "RuntimeError",
                              "msg": str(ex)})
                self._compare_saved(n, entry, None, where)
                raise
            if _is_data(ret):
                entry["ret"] = self._enc(ret, sh_ret)
            else:
                entry["ret"] = {"o": len(self.objects)}
                self.objects[len(self.objects)] = (ret, sh_ret)
            self._compare_saved(n, entry, sh_ret, where)
        else:
            saved = self.saved["entries"][n] if n < len(self.saved["entries"]) else None
            assert saved is not None and saved["call"] == entry["call"] and saved["args"] == entry["args"], (
                f"{where}: not the recorded call {saved and saved['call']} (the test changed: record the reference's "
                "answers again where oracle/_ref can be built, LT_REF_RECORD=1)")
            entry = saved
            if "raise" in entry:
                raise getattr(builtins, entry["raise"], RuntimeError)(entry["msg"])
            if isinstance(entry["ret"], dict) and "o" in entry["ret"]:
                self.objects[entry["ret"]["o"]] = (None, sh_ret)
            ret = self._dec(entry["ret"], sh_ret, self.saved["arrays"], where)
        if isinstance(entry.get("ret"), dict) and "o" in entry["ret"]:
            return _Handle(self, entry["ret"]["o"])
        return ret

    def _compare_saved(self, n, entry, sh_ret, where):
        """live and not recording: the reference's answer must be the committed one."""
        if self.recording or self.saved is None:
            return
        saved = self.saved["entries"][n] if n < len(self.saved["entries"]) else None
        msg = f"{where}: the reference's answer is not the recorded one (record again: LT_REF_RECORD=1)"
        assert saved is not None and saved["call"] == entry["call"] and saved["args"] == entry["args"], msg
        assert saved.get("raise") == entry.get("raise") and saved.get("msg") == entry.get("msg"), msg
        if "ret" in entry:
            _assert_same(self._dec(entry["ret"], sh_ret, self.arrays, where),
                         self._dec(saved["ret"], sh_ret, self.saved["arrays"], where), msg)

    def finish(self):
        if self.saved is not None and not self.recording:
            assert len(self.entries) == len(self.saved["entries"]), (
                f"{self.name}: {len(self.entries)} calls, the record has {len(self.saved['entries'])} (LT_REF_RECORD=1)")


def _assert_same(a, b, msg):
    if isinstance(a, dict):
        assert isinstance(b, dict) and list(a) == list(b), msg
        for k in a:
            _assert_same(a[k], b[k], msg)
    elif isinstance(a, (list, tuple)):
        assert type(a) is type(b) and len(a) == len(b), msg
        for x, y in zip(a, b):
            _assert_same(x, y, msg)
    else:
        x, y = np.asarray(a), np.asarray(b)
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), msg


class Reference:
    """Module stand-in: `ref.triangulate_line(...)`, `ref.OracleTriangulator(cfg)`, ..."""

    def __init__(self, record):
        self._record = record

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)
        return lambda *a, **k: self._record.call(0, name, a, k)


def recorded_tree_hashes():
    """{record name: hash of the tree oracle/_ref was built against when it was recorded}."""
    out = {}
    for f in sorted(os.listdir(RECORD_DIR)) if os.path.isdir(RECORD_DIR) else []:
        if f.endswith(".npz"):
            with np.load(os.path.join(RECORD_DIR, f)) as z:
                out[f[:-4]] = json.loads(bytes(z["__meta__"]).decode())["tree_source_hash"]
    return out
