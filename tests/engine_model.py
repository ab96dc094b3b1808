"""Plain-Python MODEL of one engine handle over its whole life (host only: no GPU, no libkdf.so).

``EngineModel(k)`` is a dict from canonical key (a Python int, ``kmer_truth.key_int``) to count plus the few bits of
state ``include/kdf.h`` names: the mode (insert / filter), ``windows``, ``key_parts`` / ``key_part``, ``hash_shift``,
``force_path``, the two upload slots, whether a loaded filter still has its sieve, and the prefilter (off / tallying /
armed, L, s and the cell tallies of ``prefilter_model``).  One method per mutator, each restating a sentence of the
header; a call the header refuses raises ``Refused(code)`` BEFORE anything is changed, so a refused call leaves the
model untouched.  The observers are computed from the dict alone.

Key extraction: the string rules of ``kmer_truth`` (any k); for k <= 63 the C oracle counts a batch (the same rules,
pinned to each other by tests/test_kmer_truth.py) because it is faster.  The key-space slice of "key_parts" is the
header's: ranges of the LOW 16 bits of the key's stored form, ``(h & 0xFFFF) * parts >> 16`` -- not
``stream_truth.slice_of``, which cuts a sorted dump by the key's own top bits.
"""
import numpy as np

import depth_truth as DT
import kmer_truth as KT
import prefilter_model as PM
from oracle import oracle as O

OK, ERR_INVALID, ERR_STATE = 0, 1, 6
SAT = (1 << 32) - 1
PF_OFF, PF_TALLYING, PF_ARMED = 0, 1, 2


class Refused(Exception):
    def __init__(self, code, why=""):
        super().__init__(f"refused ({code}): {why}")
        self.code = code


def batch_counts(reads, k):
    """{canonical key: number of valid windows} of one batch of read strings"""
    if k > 63:
        return KT.count_truth(reads, k)
    O.build()
    lo, hi, cnt = O.OracleTable(k, 1 << 12).count_reads(reads).export_ge(0)
    return {int(a) | (int(b) << 64): int(c) for a, b, c in zip(lo.tolist(), hi.tolist(), cnt.tolist())}


def slice_of_key(key, k, parts):
    """kdf.h "key_parts": the slice of a key, from the LOW 16 bits of its stored form"""
    return ((PM.stored_form(key, k) & 0xFFFF) * parts) >> 16


class EngineModel:
    def __init__(self, k):
        self.k = k
        self.long = k > 63
        self.table = {}
        self.filter_mode = False
        self.windows = 0
        self.key_parts, self.key_part = 0, 0
        self.hash_shift = 0
        self.force_path = 0
        self.fused_dump = 0
        self.sieve = False                # a loaded filter's sieve is there (force_path 4 needs it)
        self.slots = [None, None]         # upload slots: the reads they hold
        self.pf_state, self.pf_L, self.pf_s, self.pf_cells = PF_OFF, 0, 0, {}
        self.had_filter_life = False

    # ---- count -------------------------------------------------------------------------------------------------------
    def _admitted(self, key):
        if self.key_parts > 1 and slice_of_key(key, self.k, self.key_parts) != self.key_part:
            return False
        if self.pf_state == PF_ARMED:
            return min(self.pf_cells.get(PM.cell_of(key, self.k, self.pf_s), 0), 3) >= self.pf_L
        return True

    def check_count(self):
        """kdf_count_reads*: KDF_ERR_STATE while a filter is loaded and while the prefilter is tallying"""
        if self.filter_mode:
            raise Refused(ERR_STATE, "count in filter mode")
        if self.pf_state == PF_TALLYING:
            raise Refused(ERR_STATE, "count while tallying")

    def count(self, reads):
        """+1 per admitted valid window, saturating at 2^32 - 1; `windows` counts the admitted windows only"""
        self.check_count()
        for key, c in batch_counts(reads, self.k).items():
            if self._admitted(key):
                self.table[key] = min(self.table.get(key, 0) + c, SAT)
                self.windows += c

    def check_count_filtered(self, reads):
        """kdf_count_reads_filtered*: KDF_ERR_STATE without a filter, and under force_path 4 without its sieve -- the
        sieve is asked only when the stream has positions (an empty stream, no reads at all, is KDF_OK)"""
        if not self.filter_mode:
            raise Refused(ERR_STATE, "count --if in insert mode")
        if self.force_path == 4 and not self.sieve and len(reads):
            raise Refused(ERR_STATE, "force_path 4 without a sieve")

    def count_filtered(self, reads):
        """stored keys only, nothing inserted; `windows` counts every valid window; key_parts and the prefilter do not
        apply"""
        self.check_count_filtered(reads)
        for key, c in batch_counts(reads, self.k).items():
            self.windows += c
            if key in self.table:
                self.table[key] = min(self.table[key] + c, SAT)

    def upload(self, slot, reads):
        self.slots[slot] = list(reads)

    def count_uploaded(self, slot, filtered):
        """KDF_ERR_STATE on an empty slot; a call refused for the engine's mode or a tallying prefilter keeps the batch"""
        if self.slots[slot] is None:
            raise Refused(ERR_STATE, "empty slot")
        if filtered:
            self.check_count_filtered(self.slots[slot])
        else:
            self.check_count()
        reads, self.slots[slot] = self.slots[slot], None
        (self.count_filtered if filtered else self.count)(reads)

    # ---- explicit pairs ------------------------------------------------------------------------------------------------
    def add_pairs(self, keys, counts):
        """insert-or-add, both modes, never gated; counts None adds 0; a key twice in one call is summed (saturating)"""
        if len(keys):
            self.sieve = False
        for i, key in enumerate(keys):
            self.table[key] = min(self.table.get(key, 0) + (0 if counts is None else counts[i]), SAT)

    def set_counts(self, keys, counts):
        for key, c in zip(keys, counts):
            if key not in self.table:
                raise Refused(ERR_INVALID, "set_counts of a key that is not stored")
        for key, c in zip(keys, counts):
            self.table[key] = c

    def load_filter(self, keys):
        """the table becomes exactly these keys with count 0; `windows` 0; pending work dropped; prefilter untouched"""
        self.table = {key: 0 for key in keys}
        self.filter_mode, self.windows, self.sieve = True, 0, not self.long
        self.had_filter_life = True

    def reset_counts(self):
        """keys kept, counts 0, `windows` 0, the mode kept -- in insert mode too"""
        for key in self.table:
            self.table[key] = 0
        self.windows = 0

    def clear(self):
        """empty table, `windows` 0, insert mode; the prefilter (tallying or armed, with its tallies) stays"""
        self.table, self.windows, self.filter_mode, self.sieve = {}, 0, False, False

    # ---- options -------------------------------------------------------------------------------------------------------
    def set_option(self, name, value):
        """no option changes the contents; the refusals are those kdf.h lists"""
        if name == "key_parts" or name == "key_part":
            parts = value if name == "key_parts" else self.key_parts
            part = value if name == "key_part" else self.key_part
            if value < 0 or parts > 65536 or (name == "key_part" and part >= max(parts, 1)):
                raise Refused(ERR_INVALID, name)
            if parts > 1 and self.pf_state != PF_OFF:
                raise Refused(ERR_STATE, "key_parts with a prefilter")
            self.key_parts, self.key_part = parts, (0 if name == "key_parts" else part)
        elif name == "force_path":
            if value not in (0, 1, 2, 4) or (self.long and value in (2, 4)):
                raise Refused(ERR_INVALID, "force_path")
            self.force_path = value
        elif name == "hash_shift":
            if value > 8 or (value != 0 and self.long):
                raise Refused(ERR_INVALID, "hash_shift")
            if value != 0 and self.pf_state != PF_OFF:
                raise Refused(ERR_STATE, "hash_shift with a prefilter")
            if value != self.hash_shift and self.table:
                raise Refused(ERR_STATE, "hash_shift on a table that holds keys")
            self.hash_shift = value
        elif name == "fused_dump":
            if value and self.long:
                raise Refused(ERR_INVALID, "fused_dump")
            self.fused_dump = int(value != 0)
        elif name == "big_bucket_log2cap":
            if not 10 <= value <= 64:
                raise Refused(ERR_INVALID, name)
        elif name == "binned_max_positions":
            if not 64 <= value <= 1 << 31:
                raise Refused(ERR_INVALID, name)

    # ---- prefilter -----------------------------------------------------------------------------------------------------
    def prefilter_begin(self, L, s):
        if self.pf_state != PF_OFF:
            raise Refused(ERR_STATE, "begin: not off")
        if L not in (2, 3) or not (s == 0 or 16 <= s <= 38):
            raise Refused(ERR_INVALID, "begin: arguments")
        if self.key_parts > 1 or self.hash_shift:
            raise Refused(ERR_STATE, "begin with key_parts / hash_shift")
        assert s != 0, "the model takes an explicit log2_cells"
        self.pf_state, self.pf_L, self.pf_s, self.pf_cells = PF_TALLYING, L, s, {}

    def check_tallying(self):
        if self.pf_state != PF_TALLYING:
            raise Refused(ERR_STATE, "not tallying")

    def prefilter_add(self, reads):
        self.check_tallying()
        for key, c in batch_counts(reads, self.k).items():
            cell = PM.cell_of(key, self.k, self.pf_s)
            self.pf_cells[cell] = self.pf_cells.get(cell, 0) + c

    def prefilter_add_uploaded(self, slot):
        self.check_tallying()
        if self.slots[slot] is None:
            raise Refused(ERR_STATE, "empty slot")
        reads, self.slots[slot] = self.slots[slot], None
        self.prefilter_add(reads)

    def prefilter_arm(self):
        self.check_tallying()
        self.pf_state = PF_ARMED

    def prefilter_drop(self):
        if self.pf_state == PF_OFF:
            raise Refused(ERR_STATE, "drop: off")
        self.pf_state, self.pf_cells = PF_OFF, {}

    def prefilter_fill(self):
        if self.pf_state == PF_OFF:
            raise Refused(ERR_STATE, "fill: off")
        by = [0, 0, 0, 0]
        for v in self.pf_cells.values():
            by[min(v, 3)] += 1
        by[0] = (1 << self.pf_s) - len(self.pf_cells)
        return by

    # ---- observers -----------------------------------------------------------------------------------------------------
    def stats(self):
        return len(self.table), self.windows

    def count_ge(self, m):
        return sum(1 for c in self.table.values() if c >= m)

    def export_ge(self, m):
        ks = sorted(key for key, c in self.table.items() if c >= m)
        return ks, np.array([self.table[key] for key in ks], dtype=np.uint32)

    def query(self, keys):
        return np.array([self.table.get(key, 0) for key in keys], dtype=np.uint32)

    def histogram(self, high):
        bins = np.zeros(high + 2, np.uint64)
        for c in self.table.values():
            bins[min(c, high + 1)] += 1
        return bins

    def count_stats(self):
        cs = list(self.table.values())
        return {"unique": sum(1 for c in cs if c == 1), "distinct": sum(1 for c in cs if c >= 1), "total": sum(cs),
                "max_count": max(cs, default=0)}

    def note_scan(self, reads):
        """a scan (non-empty stream, not force_path 1, k <= 63) rebuilds the sieve that kdf_add_pairs* dropped"""
        if self.filter_mode and not self.long and self.force_path != 1 and len(reads):
            self.sieve = True

    def scan(self, reads):
        """-> (hit words over the stream of `reads`, distinct hit keys per read)"""
        hits, distinct = KT.scan_truth(reads, self.k, self.table)
        offs = DT.offsets_of(reads)
        return KT.hit_words(offs, hits, (int(offs[-1]) + 63) // 64 + 2), distinct

    def window_counts(self, reads):
        counts, valid, _ = DT.profile(reads, self.k, self.table)
        return counts, valid

    def read_depth(self, reads, low_max):
        return DT.depth_rows(reads, self.k, self.table, low_max)
