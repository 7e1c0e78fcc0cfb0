"""A plain-Python statement of the mate pairing of `sam to [interleaved] raw|fasta|fastq` (src/sam_to_fastq.rs:100-137) over
(flag, qname) records: which record's text goes to which of the three outputs, in which order.  The two HashMaps of the reference are
two dicts here; a dict keeps its keys in insertion order and an assignment to a key that is present keeps its place, which is this
build's rule for the leftovers (the reference iterates its maps in arbitrary order)."""


def kind(flag):
    """None: the loop writes the record nowhere whatever comes; 0 not paired, 1 first in template, 2 last in template"""
    if flag & 0x100 or flag & 0x800:                                    # :101
        return None
    if not flag & 0x1:                                                  # :113
        return 0
    if flag & 0x40:                                                     # :115 (is_first_in_template is asked first)
        return 1
    if flag & 0x80:                                                     # :122
        return 2
    return None


def pair(records):
    """records: (flag, qname) in file order.  Returns (out_1, out_2, out_single): lists of record indices in the order their texts
    are written; out_1[p] and out_2[p] are the two mates of pair p."""
    return _loop(records)[:3]


def _loop(records):
    reads_1, reads_2 = {}, {}                                           # qname -> index of the record whose text is pending
    out_1, out_2, out_single = [], [], []
    for i, (flag, qname) in enumerate(records):
        k = kind(flag)
        if k is None:
            continue
        if k == 0:
            out_single.append(i)                                        # :114
        elif k == 1:
            if qname in reads_2:                                        # :116-118
                out_1.append(i)
                out_2.append(reads_2.pop(qname))
            else:
                reads_1[qname] = i                                      # :120 insert replaces the value
        else:
            if qname in reads_1:                                        # :123-125
                out_1.append(reads_1.pop(qname))
                out_2.append(i)
            else:
                reads_2[qname] = i                                      # :127
    n_single = len(out_single)
    out_single += list(reads_1.values()) + list(reads_2.values())       # :134-136
    return out_1, out_2, out_single, n_single, len(reads_1), len(reads_2)


def interleave(out_1, out_2):
    """the one stream of interleaved mode, where out_1 and out_2 are both stdout: pair p's first mate, then its last mate"""
    return [i for p in zip(out_1, out_2) for i in p]


def counts(records):
    """what sk_bam_file_pairs reports: pairs, unpaired, leftover first mates, leftover last mates, paired records written nowhere"""
    out_1, _, _, n_single, n_left_1, n_left_2 = _loop(records)
    paired = sum(1 for flag, _ in records if kind(flag) in (1, 2))
    return [len(out_1), n_single, n_left_1, n_left_2, paired - 2 * len(out_1) - n_left_1 - n_left_2]
