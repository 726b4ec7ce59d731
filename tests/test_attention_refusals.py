"""CPU: what the eight attention entry points refuse, one table for all of them.  Every case changes one argument of a good call
and is refused on the host, before a launch, with MI_ERR_ARG and a message that starts with the entry point's name and carries the
key word of the check (fake pointers: nothing is dereferenced, and only refused calls are made)."""
import pytest

FAKE = 0x10000  # non-null, 16-byte aligned, never dereferenced
ARG = -1        # MI_ERR_ARG
FWD = (("q", "k", "v", "o", "lse"), ("q_ts", "k_ts", "v_ts", "o_ts"))
BWD = (("q", "k", "v", "o", "dout", "lse", "delta", "dq", "dk", "dv"),
       ("q_ts", "k_ts", "v_ts", "o_ts", "do_ts", "dq_ts", "dk_ts", "dv_ts"))
SHORT_BWD = (tuple(p for p in BWD[0] if p != "delta"), BWD[1])
LONG_S, SHORT_S = (0, 64, 112, 120, 136, 200), (0, 8, 24, 120, 128)
# entry point: ((pointers, strides), arguments between `causal` and the stream, a good S, the S refused, must be causal).
# The K / V stride that puts one batch at or past 2 GiB (S * stride * 2 bytes >= 2^31) is 1 << 23 at S = 256; the short launchers
# take no S above 112, where 1 << 23 is still below the limit (and would be launched): theirs is 1 << 24.
ENTRIES = {
    "mi_attn_fwd": (FWD, (), 256, LONG_S, False),
    "mi_attn_bwd": (BWD, (), 256, LONG_S, False),
    "mi_attn_fwd_win": (FWD, ("window",), 256, LONG_S, True),
    "mi_attn_bwd_win": (BWD, ("window",), 256, LONG_S, True),
    "mi_attn_fwd_seg": (FWD, ("seg_start", "seg_end"), 256, LONG_S, True),
    "mi_attn_bwd_seg": (BWD, ("seg_start", "seg_end"), 256, LONG_S, True),
    "mi_attn_short_fwd": (FWD, (), 80, SHORT_S, True),
    "mi_attn_short_bwd": (SHORT_BWD, (), 80, SHORT_S, True),
}


@pytest.mark.parametrize("name", list(ENTRIES))
def test_host_refusals(name):
    from llm_fp8_amd import _lib as L
    (ptrs, strides), extra, good_s, bad_s, needs_causal = ENTRIES[name]
    lib = L.load()

    def refused(word, **over):
        a = dict({p: FAKE for p in ptrs}, B=1, S=good_s, H=4, G=2, D=64, scale=0.125, causal=1, window=32, seg_start=FAKE,
                 seg_end=FAKE, **{s: 512 for s in strides})
        a.update(over)
        rc = getattr(lib, name)(*[a[p] for p in ptrs], a["B"], a["S"], a["H"], a["G"], a["D"], *[a[s] for s in strides],
                                a["scale"], a["causal"], *[a[e] for e in extra], None)
        msg = lib.mi_last_error().decode()
        assert rc == ARG and msg.startswith(name + ":") and word in msg, (over, rc, msg)

    for p in ptrs:
        refused("null", **{p: None})
        if p not in ("lse", "delta"):  # the 16-byte operands
            refused("aligned", **{p: FAKE + 8})
    for S in bad_s:
        refused("seq", S=S)
    for D in (0, 32, 96, 256):
        refused("head_dim", D=D)
    refused("B/H/G", H=4, G=3)
    refused("B/H/G", B=0)
    for s in strides:
        refused("strides", **{s: 516})
    big = 1 << 24 if name.startswith("mi_attn_short") else 1 << 23
    assert good_s * big * 2 >= 2 ** 31
    refused("2 GiB", k_ts=big)
    refused("2 GiB", v_ts=big)
    if name.startswith("mi_attn_short"):
        refused("grid", H=65536, G=65536)
    else:
        refused("grid", H=65536, G=1)
    if needs_causal:
        refused("causal", causal=0)
    if "window" in extra:
        for window in (0, -1, -(2 ** 31)):
            refused("window", window=window)
    for p in extra:
        if p.startswith("seg_"):
            refused("null", **{p: None})
            refused("aligned", **{p: FAKE + 2})
