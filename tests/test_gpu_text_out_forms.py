"""The rules every verb that assembles a text on the device shares (replace_text, filter_text,
route_text, range_text, extract_text, fields_text), pinned once per verb on a text of a few lines:
out= together with out_cap= (the room is the smaller of the two), what an unusable out= or a
non-contiguous device text is answered with, and the host form's second call, when the output is
longer than the first guess of len + 64 bytes.  The expectations are the per-verb modules' own,
from the oracle."""
import numpy as np
import pytest

import one_amd
from one_amd import workloads as W
from golden_util import load_dfa

import range_rule as R
import test_gpu_extract_text as XT
import test_gpu_fields_text as FD
import test_gpu_filter_text as FT
import test_gpu_range_text as RG
import test_gpu_replace_text as RP
import test_gpu_route_text as RO

pytestmark = pytest.mark.gpu

SENT = 0x55
VERBS = ["replace_text", "filter_text", "route_text", "range_text", "extract_text", "fields_text"]

_cases = {}


class _Case:
    """one verb on one small text: call(data, **room) is the verb with the case's arguments,
    out_len and out are got[len_at] and got[out_at] of its device tuple, want the bytes expected"""

    def __init__(self, exe, text, want, call, len_at):
        assert len(text) < 200 and len(want) >= 16, (len(text), len(want))
        self.exe, self.text, self.want, self.call = exe, text, want, call
        self.len_at, self.out_at = len_at, len_at + 1


def _replace_text():
    text = b"ab 12345a cd 12345a\nnothing in this line\n12345a12345a ef\ntail 12345a"
    exe = one_amd.Executable(load_dfa("num3"))
    want = RP._want("num3", text, b"<#>").out[0]
    return _Case(exe, text, want, lambda d, **kw: one_amd.replace_text(exe, d, b"<#>", **kw), 2)


def _filter_text():
    text = b"one aab\ntwo\nthree\nfour aab aab\nfive\nsix\nseven aab\ntail aab"
    exe = one_amd.Executable(load_dfa("aab"))
    want = FT._expect("aab", text, 4, 1, False, 1, 0).out
    return _Case(exe, text, want,
                 lambda d, **kw: one_amd.filter_text(exe, d, 4, True, before=1, **kw), 3)


def _route_text():
    text = b"one aab\ntwo\nthree\nfour aab aab\nfive\nsix\nseven aab\ntail aab"
    exe = one_amd.Executable(load_dfa("aab"))
    want = RO._expect("aab", text, 2).out
    return _Case(exe, text, want, lambda d, **kw: one_amd.route_text(exe, d, 2, **kw), 4)


def _range_text():
    heads = W.log100_heads()
    o, c = RG._border_results()
    text = (b"before\nzz " + heads[RG.OPEN_HEAD] + b"qq\nbody one\nbody two\nzz " +
            heads[RG.CLOSE_HEAD] + b"qq\nafter\ntail")
    exe = one_amd.Executable(load_dfa("log100"))
    want = R.expect("log100", text, o, c).out
    return _Case(exe, text, want, lambda d, **kw: one_amd.range_text(exe, d, o, c, **kw), 3)


def _extract_text():
    text = b"ab 12345a cd 12345a\nnothing in this line\n12345a12345a ef\ntail 12345a"
    exe = one_amd.Executable(load_dfa("num3"))
    want = XT._oracle("num3", text).out()[1]
    return _Case(exe, text, want, lambda d, **kw: one_amd.extract_text(exe, d, **kw), 2)


def _fields_text():
    text = b"a,bb,ccc,dddd\nno separator\n,x,,y,\n1,2,3,4,5,6\ntail,of,the,text"
    exe = one_amd.Executable(FD._blob("comma"))
    want = FD._oracle("comma", text).out("1,3-", 0, False, b" ")[3]
    return _Case(exe, text, want, lambda d, **kw: one_amd.fields_text(exe, d, "1,3-", **kw), 3)


def _case(verb):
    if verb not in _cases:
        _cases[verb] = globals()["_" + verb]()
    return _cases[verb]


def _dev(text):
    import torch
    return torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).cuda()


@pytest.mark.parametrize("verb", VERBS)
def test_out_and_out_cap_together(verb):
    """the room is min(out_cap, out.numel()): nothing behind it is written, out_len is the whole
    length, and the tensor handed in is the one that comes back"""
    import torch
    x = _case(verb)
    n = len(x.want)
    dev = _dev(x.text)
    for cap, written in ((n // 2, n // 2), (1, 1), (n - 1, n - 1), (n + 100, n)):
        out = torch.full((n + 5,), SENT, dtype=torch.uint8, device="cuda")
        got = x.call(dev, out=out, out_cap=cap)
        torch.cuda.synchronize()
        assert got[x.out_at] is out, (verb, cap)
        assert got[x.len_at].item() == n, (verb, cap, got[x.len_at].item(), n)
        mine = out.cpu().numpy().tobytes()
        assert mine[:written] == x.want[:written], (verb, cap)
        assert mine[written:] == bytes([SENT]) * (n + 5 - written), (verb, cap)


@pytest.mark.parametrize("verb", VERBS)
def test_unusable_out_is_refused(verb):
    """out= must be a contiguous uint8 CUDA tensor: a CPU tensor, another dtype and a strided view
    are refused, with and without out_cap"""
    import torch
    x = _case(verb)
    n = len(x.want)
    dev = _dev(x.text)
    bad = {"cpu": torch.zeros(n, dtype=torch.uint8),
           "dtype": torch.zeros(n, dtype=torch.int8, device="cuda"),
           "strided": torch.zeros(2 * n, dtype=torch.uint8, device="cuda")[::2]}
    assert not bad["strided"].is_contiguous()
    for what, out in bad.items():
        for kw in (dict(out=out), dict(out=out, out_cap=n)):
            with pytest.raises(one_amd.RedExceptApi, match="out must be a contiguous uint8 CUDA"):
                x.call(dev, **kw)
    torch.cuda.synchronize()
    assert not bad["cpu"].any() and not bad["dtype"].any() and not bad["strided"].any(), verb


@pytest.mark.parametrize("verb", VERBS)
def test_strided_device_text_is_refused(verb):
    import torch
    x = _case(verb)
    wide = torch.zeros(2 * len(x.text), dtype=torch.uint8, device="cuda")
    wide[::2] = _dev(x.text)
    out = torch.full((len(x.want),), SENT, dtype=torch.uint8, device="cuda")
    with pytest.raises(one_amd.RedExceptApi, match="device input must be a contiguous uint8 CUDA"):
        x.call(wide[::2], out=out)
    with pytest.raises(one_amd.RedExceptApi, match="device input must be a contiguous uint8 CUDA"):
        x.call(wide[::2], out_cap=len(x.want))
    torch.cuda.synchronize()
    assert (out == SENT).all(), verb


@pytest.mark.parametrize("verb", VERBS)
def test_host_text_takes_no_out(verb):
    x = _case(verb)
    for kw in (dict(out_cap=len(x.want)), dict(out=np.zeros(len(x.want), dtype=np.uint8))):
        with pytest.raises(one_amd.RedExceptApi, match="go with a CUDA tensor text"):
            x.call(x.text, **kw)


def test_replace_text_host_form_second_call():
    """a 40-byte repl: the output is longer than len + 64, the host form asks once more"""
    text, repl = b"12345a " * 20 + b"\nno match\n12345a", RP.REPLS[3]
    w = RP._want("num3", text, repl)
    assert len(text) < 200 and len(w.out[0]) > len(text) + 64 and w.n_replaced == 20
    got = one_amd.replace_text(one_amd.Executable(load_dfa("num3")), text, repl)
    assert got == (w.n_lines, w.n_replaced, w.out[0])


def test_extract_text_host_form_second_call():
    """adjacent three-byte matches (no golden DFA has shorter ones): every piece brings a
    delimiter, so a line of 100 of them comes out a third longer"""
    text = b"aab" * 100 + b"\nnone\n"
    x = XT._oracle("aab", text)
    n, want = x.out()
    assert n == 100 and want == b"aab\n" * 100 and len(want) > len(text) + 64
    got = one_amd.extract_text(one_amd.Executable(load_dfa("aab")), text)
    assert got == (x.n_lines, n, want)


def test_fields_text_host_form_second_call():
    """an 8-byte sep between one-byte fields: the output is longer than len + 64"""
    text, sep = b"a," * 60 + b"z\nno separator\n", b"12345678"
    want = FD._oracle("comma", text).out("1-", 0, False, sep)
    assert len(text) < 200 and len(want[3]) > len(text) + 64 and want[2] == 62
    got = one_amd.fields_text(one_amd.Executable(FD._blob("comma")), text, "1-", sep=sep)
    assert got == want
