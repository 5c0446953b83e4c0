"""Loaders for the committed golden fixtures (tests/golden/, made by oracle/gen_golden.py)."""
import base64
import json
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
STYLES = ["instant", "first", "tangent", "last", "full"]
CONFIG_DFAS = ["err", "uri", "log100", "syn256", "num3", "newyork", "aab", "dotstar_err",
               "uri_v6", "uri_user", "syn4k"]


def unb64(s):
    return base64.b64decode(s)


def load_kat():
    with open(os.path.join(GOLD, "kat_matcher.json")) as f:
        return json.load(f)


def kat_items():
    """Yields (case_name, fmt_name, blob, calls) for every KAT case x format that compiled."""
    for case in load_kat()["cases"]:
        for fmt, b in case["blobs"].items():
            if "reda" in b:
                yield case["name"], fmt, unb64(b["reda"]), case["calls"]


def load_omnibus():
    with open(os.path.join(GOLD, "omnibus.json")) as f:
        meta = json.load(f)
    blobs = np.load(os.path.join(GOLD, "omnibus_blobs.npz"))
    return meta["rows"], blobs


_DFA_CACHE = {}


def load_dfa(name):
    """The reference-compiled blob of a config DFA (big ones are stored xz-compressed)."""
    if name not in _DFA_CACHE:
        path = os.path.join(GOLD, "dfas", name + ".reda")
        if os.path.exists(path):
            with open(path, "rb") as f:
                _DFA_CACHE[name] = f.read()
        else:
            import lzma
            with open(path + ".xz", "rb") as f:
                _DFA_CACHE[name] = lzma.decompress(f.read())
    return _DFA_CACHE[name]


def load_vectors(name):
    return np.load(os.path.join(GOLD, "vectors_%s.npz" % name))


def expect_of(vec, verb, style_idx, lead):
    key = "%s_%d_%d" % (verb, style_idx, lead)
    res = vec[key + "_res"]
    if verb in ("match", "search"):
        return res, vec[key + "_start"], vec[key + "_end"]
    return res, None, None


# The long-text verbs scan their per-chunk values in blocks of 1024 chunks and the block totals in
# rounds of 1024 blocks: more than 1024 * 1024 chunks put the second round's carry to work.
SCAN_ROUND = 1024 * 1024
_SCAN_TEXT = []


def scan_round_text():
    """(text, chunk_bytes, border): 16 * (2^20 + 1025) + 5 fill bytes 0x01 - 1,049,602 chunks of 16,
    1,026 blocks - with "New York" every 4,096 bytes, plant k shifted by k % 16 so the plants
    straddle chunk borders at every offset; border = the first byte of chunk 1024 * 1024"""
    if not _SCAN_TEXT:
        chunk = 16
        n = chunk * (SCAN_ROUND + 1025) + 5
        a = np.full(n, 0x01, dtype=np.uint8)
        piece = np.frombuffer(b"New York", dtype=np.uint8)
        for k, b in enumerate(range(4096, n, 4096), 1):
            at = b + k % 16
            if at + len(piece) <= n:
                a[at:at + len(piece)] = piece
        assert (n + chunk - 1) // chunk == 1049602 and (1049602 + 1023) // 1024 == 1026
        _SCAN_TEXT.append((bytes(a), chunk, chunk * SCAN_ROUND))
    return _SCAN_TEXT[0]


def literal_dfa(word):
    """anchored `word` as a blob: 0 = error (pure dead end), 1 = initial, 2.. = its prefixes, the
    last accepts (every byte -> error)"""
    from oracle.reda_writer import write_reda
    equiv = np.zeros(256, dtype=np.uint8)
    for k, ch in enumerate(sorted(set(word)), 1):
        equiv[ch] = k
    trans = np.zeros((len(word) + 2, int(equiv.max()) + 1), dtype=np.int64)
    for k, ch in enumerate(word):
        trans[1 + k, equiv[ch]] = 2 + k
    result = np.zeros(len(word) + 2, dtype=np.int64)
    result[-1] = 1
    return write_reda(trans, result, equiv=equiv, initial=1)
