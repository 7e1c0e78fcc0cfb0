"""CPU: tests/bam_pair_model.py — the loop of src/sam_to_fastq.rs:100-137 over (flag, qname) — on cases derived by hand."""
from tests import bam_pair_model as pm

F1, F2, REV, SEC, SUP = 1 | 0x40, 1 | 0x80, 0x10, 0x100, 0x800


def test_first_then_last_and_last_then_first():
    assert pm.pair([(F1, b"a"), (F2, b"a")]) == ([0], [1], [])
    assert pm.pair([(F2, b"a"), (F1, b"a")]) == ([1], [0], [])           # the first mate's text still goes to output 1


def test_pairs_are_ordered_by_the_record_that_completes_them():
    recs = [(F1, b"a"), (F1, b"b"), (F2, b"b"), (F2, b"a")]
    assert pm.pair(recs) == ([1, 0], [2, 3], [])
    assert pm.interleave(*pm.pair(recs)[:2]) == [1, 2, 0, 3]


def test_a_second_insert_replaces_the_first():
    assert pm.pair([(F1, b"a"), (F1, b"a"), (F2, b"a")]) == ([1], [2], [])          # record 0 is written nowhere
    assert pm.counts([(F1, b"a"), (F1, b"a"), (F2, b"a")]) == [1, 0, 0, 0, 1]
    assert pm.pair([(F2, b"a"), (F2, b"a"), (F1, b"a")]) == ([2], [1], [])


def test_a_third_record_is_a_leftover_with_a_new_order():
    # b enters reads_1 before a's third record does: a was removed by the pair, so its new entry comes behind b's
    recs = [(F1, b"a"), (F1, b"b"), (F2, b"a"), (F1, b"a")]
    assert pm.pair(recs) == ([0], [2], [1, 3])
    assert pm.counts(recs) == [1, 0, 2, 0, 0]


def test_a_replaced_entry_keeps_the_order_of_its_first_insert():
    recs = [(F1, b"a"), (F1, b"b"), (F1, b"a")]
    assert pm.pair(recs) == ([], [], [2, 1])                             # a's text is record 2's, its place record 0's
    assert pm.counts(recs) == [0, 0, 2, 0, 1]


def test_both_mate_flags_count_as_first():
    assert pm.kind(1 | 0x40 | 0x80) == 1
    assert pm.pair([(1 | 0x40 | 0x80, b"a"), (F2, b"a")]) == ([0], [1], [])
    assert pm.pair([(1 | 0x40 | 0x80, b"a"), (F1, b"a")]) == ([], [], [1])


def test_paired_with_neither_mate_flag_is_dropped():
    assert pm.kind(1) is None and pm.kind(1 | REV) is None
    assert pm.pair([(F1, b"a"), (1, b"a"), (F2, b"a")]) == ([0], [2], [])
    assert pm.counts([(1, b"a")]) == [0, 0, 0, 0, 0]


def test_secondary_and_supplementary_between_mates_are_skipped():
    recs = [(F1, b"a"), (F2 | SEC, b"a"), (F1 | SUP, b"a"), (SEC, b"a"), (F2, b"a")]
    assert pm.pair(recs) == ([0], [4], [])


def test_unpaired_records_go_to_the_single_output_in_file_order_before_the_leftovers():
    recs = [(F2, b"x"), (0, b"u"), (F1, b"a"), (REV, b"a"), (F2, b"a"), (0, b"x")]
    assert pm.pair(recs) == ([2], [4], [1, 3, 5, 0])
    assert pm.counts(recs) == [1, 3, 0, 1, 0]


def test_leftover_first_mates_come_before_leftover_last_mates():
    recs = [(F2, b"p"), (F1, b"q"), (F2, b"r"), (F1, b"s")]
    assert pm.pair(recs) == ([], [], [1, 3, 0, 2])
    assert pm.counts(recs) == [0, 0, 2, 2, 0]


def test_names_are_whole_names():
    recs = [(F1, b"a"), (F2, b"a/2"), (F2, b"ab"), (F2, b"")]
    assert pm.pair(recs) == ([], [], [0, 1, 2, 3])
