"""CPU: the host rules of the tracer -- what the next call's list capacity and compact rows are, decoded from the mirrored counter words
(envgs_amd.tracing.decode_counters, CapState.next_rows).  Expected values are worked by hand from the rules as the docstrings state them."""
import pytest

from envgs_amd import _lib, tracing


def _words(max_list=0, found=0, hits=0, filed=0, entries=0):
    w = [0] * _lib.TRACE_COUNTER_MIRROR
    w[_lib.CTR_MAX_LIST] = max_list
    for tot, v in ((_lib.TOT_FOUND, found), (_lib.TOT_HITS, hits)):
        lo, hi = v & 0xFFFFFFFF, v >> 32
        w[_lib.CTR_TOTALS + 2 * tot] = lo - (1 << 32) if lo >= (1 << 31) else lo       # (the mirror is int32: a low word above 2^31 reads negative)
        w[_lib.CTR_TOTALS + 2 * tot + 1] = hi
    w[_lib.CTR_SPARSE_FILED], w[_lib.CTR_BATCH_ENTRIES] = filed, entries
    return w


# 20 % + 8, up to a multiple of 64: 0 -> 8 -> 64; 100 -> 128 -> 128; 220 -> 272 -> 320, but 220 * 1.1 + 8 = 250 <= 256 keeps the class;
# 240 -> 296 -> 320 and 240 * 1.1 + 8 = 272 > 256; 2000 -> 2408 -> clamped to 1024
@pytest.mark.parametrize("longest,cap", [(0, 64), (100, 128), (220, 256), (240, 320), (2000, 1024)])
def test_capacity_follows_the_longest_list(longest, cap):
    assert tracing.decode_counters(_words(max_list=longest), 1)[0] == cap


def test_totals_are_reassembled_from_their_words():
    found, hits = (3 << 32) + 0x90000005, 7_000_000
    cap, per_ray, per_entry = tracing.decode_counters(_words(max_list=100, found=found, hits=hits, filed=1000, entries=3000), 1 << 20)
    assert cap == 128 and per_ray == found / (1 << 20) and per_entry == hits / 4000
    assert tracing.decode_counters(_words(found=10_000), 1000)[1:] == (10.0, None)              # no entries: nothing known about coherence
    assert tracing.decode_counters(_words(found=5), 0)[1] == 5.0                                # (an empty call divides by 1)


def test_rows_follow_the_hits_found_per_ray():
    st = tracing.CapState()
    assert st.next_rows(1000, 256) == 196096            # first call: 192 per ray -> 192000 + 4096
    st.found_per_ray = 10.0
    assert st.next_rows(1000, 256) == 19596             # 1.15 * 10 + 4 = 15.5 per ray -> 15500 + 4096
    assert st.next_rows(10, 64) == 640                  # never more than the (R, cap) layout: 10 * 64 < 155 + 4096


def test_forced_capacity_and_rows_override_both_rules(monkeypatch):
    st = tracing.CapState()
    st.found_per_ray = 10.0
    monkeypatch.setitem(tracing.HIT_CAP, "force", 24)
    assert st.next_cap(None) == 24 and st.cap == 512                   # (returned, not adopted; no device is asked for anything)
    monkeypatch.setitem(tracing.ROW_CAP, "force_per_ray", 2)
    assert st.next_rows(1000, 256) == 2 * 1000 + 4096
    monkeypatch.setitem(tracing.ROW_CAP, "force_per_ray", 0)
    assert st.next_rows(1000, 256) == 4096
