"""--meta --amplicon-depth / --mask-reads-relative-frequency / --mask-seeds-relative-frequency: the restatement the tests compare
the product with, and the read family dealt into amplicons.  No product code in here: the file rules and the grouping are the
reference's (extractReadSequences, src/mgsr.cpp:1216-1342), the per-group rule is mask_checks.merge_lists and
mask_checks.restate_masks applied group by group with the thresholds of src/mgsr.cpp:2062-2075 and concatenated in group order.

The rule: the file maps read ids to primer ids; groups are numbered by first appearance of the primer id, a read listed twice
belongs to the primer of its last line, a read that is not listed belongs to one more group, the last.  Reads are merged by
seedmer list within their group; count[g][h] is over the merged reads of g; the threshold of a listed group is the absolute
parameter, or int(rf * N_g) under a relative one (N_g: the group's raw reads); the last group always takes the absolute one."""
import functools

import numpy as np

import mask_checks as mc


def parse_table(text):
    """the file's text -> (primer ids by first appearance, {read id: group}); ValueError(line number) for a malformed line"""
    names, group_of, of_read = [], {}, {}
    for number, line in enumerate(text.split("\n"), 1):
        line = line.rstrip("\r")
        if not line:
            continue
        fields = line.split("\t")
        if len(fields) != 2 or not fields[0] or not fields[1]:
            raise ValueError(number)
        if fields[1] not in group_of:
            group_of[fields[1]] = len(names)
            names.append(fields[1])
        of_read[fields[0]] = group_of[fields[1]]
    return names, of_read


def groups_of(read_names, n_groups, of_read):
    """the group of every named raw read: an unlisted one belongs to group n_groups"""
    return np.array([of_read.get(x, n_groups) for x in read_names], np.int32)


def thresholds(n_raw, mask_reads=0, mask_seeds=0, reads_rf=0.0, seeds_rf=0.0):
    """(whole reads?, [T_g]) for groups with n_raw raw reads, the unlisted group last (src/mgsr.cpp:2049-2053, 2062-2075)"""
    assert sum(x > 0 for x in (mask_reads, mask_seeds, reads_rf, seeds_rf)) <= 1, "Only one masking parameter can be set at a time"
    whole = mask_reads > 0 or reads_rf > 0
    absolute, rf = (mask_reads, reads_rf) if whole else (mask_seeds, seeds_rf)
    t = [int(float(rf) * float(n)) if rf > 0 else int(absolute) for n in n_raw]       # the double product, truncated
    t[-1] = int(absolute)
    return whole, t


def restate_groups(merged, n_raw, mask_reads=0, mask_seeds=0, reads_rf=0.0, seeds_rf=0.0):
    """merged[g] = (offsets, hashes, orientations, multiplicities) of group g before masking, n_raw[g] its raw reads ->
    dict(lists, mult, amplicons, old_to_new (per group: merged read before -> merged read of the whole result, -1 = dropped),
    info (N_g, T_g, before, left per group), triples [(g, h, count)] ascending, counts {h: sum over groups}, reads_dropped,
    seeds_removed).  With no parameter above 0 nothing is masked and `triples` / `counts` still describe the groups."""
    whole, thr = thresholds(n_raw, mask_reads, mask_seeds, reads_rf, seeds_rf)
    off, hh, vv, mm, amps, maps, info, triples, totals = [0], [], [], [], [], [], [], [], {}
    dropped = removed = 0
    for g, (o, h, v, m) in enumerate(merged):
        w_off, w_h, w_v, w_m, to, nd, nr, counts = mc.restate_masks(o, h, v, m, thr[g] if whole else 0, 0 if whole else thr[g])
        maps.append(np.where(to >= 0, to + len(mm), -1))
        hh += w_h.tolist(); vv += w_v.tolist(); mm += w_m.tolist()
        off += (w_off[1:] + off[-1]).tolist()
        amps += [g] * len(w_m)
        info.append((int(n_raw[g]), thr[g], len(m), len(w_m)))
        triples += [(g, x, counts[x]) for x in sorted(counts)]
        for x, c in counts.items():
            totals[x] = totals.get(x, 0) + c
        dropped += nd
        removed += nr
    return dict(lists=(np.array(off, np.int64), np.array(hh, np.uint64), np.array(vv, np.uint8)), mult=np.array(mm, np.int64),
                amplicons=np.array(amps, np.int32), old_to_new=maps, info=info, triples=triples, counts=totals, reads_dropped=dropped,
                seeds_removed=removed)


def merge_by_group(reads, groups, n_groups):
    """raw reads with their groups -> (merged[g] as restate_groups takes it, n_raw[g], per raw read (g, merged read within g
    or -1)); group n_groups, the unlisted one, last"""
    merged, n_raw, where = [], [], [None] * len(reads)
    for g in range(n_groups + 1):
        members = [i for i in range(len(reads)) if groups[i] == g]
        o, h, v, m, to = mc.merge_lists([reads[i] for i in members])
        merged.append((o, h, v, m))
        n_raw.append(len(members))
        for i, t in zip(members, to.tolist()):
            where[i] = (g, t)
    return merged, n_raw, where


def raw_to_merged(where, old_to_new):
    return np.array([old_to_new[g][t] if t >= 0 else -1 for g, t in where], np.int64)


class Dealt:
    """names / reads: the raw reads in a shuffled order; table: the file's text; group_names; groups: per raw read"""


@functools.lru_cache(maxsize=None)
def family():
    """mask_checks.family() dealt into amplicons, each read with a name of its own.  amp_1: tiles[0:30], the triplicated reads
    once, mutated[0:5] (40 raw reads); amp_2: tiles[30:60], the triplicated reads again (five lists sit in two groups), the
    reverse complements, mutated[5:10] (48); amp_3: the tandem read twice and the one-seedmer read (3); amp_empty: listed only
    for a read id that is not in the sample; unlisted: the isolated windows, the 2,000-base window and the 20 kb read."""
    F = mc.family()
    named = {}
    named["amp_1"] = ([("tile%02d" % i, r) for i, r in enumerate(F.tiles[:30])] + [("tripA%d" % i, r) for i, r in enumerate(F.triplicated)] +
                      [("mut%d" % i, r) for i, r in enumerate(F.mutated[:5])])
    named["amp_2"] = ([("tile%02d" % (30 + i), r) for i, r in enumerate(F.tiles[30:])] + [("tripB%d" % i, r) for i, r in enumerate(F.triplicated)] +
                      [("rc%d" % i, r) for i, r in enumerate(F.revcomp)] + [("mut%d" % (5 + i), r) for i, r in enumerate(F.mutated[5:])])
    named["amp_3"] = [("tandem0", F.tandem), ("tandem1", F.tandem), ("single", F.single)]
    unlisted = [("iso%d" % i, r) for i, r in enumerate(F.isolated)] + [("window", F.window), ("long", F.long)]
    assert [len(named[x]) for x in ("amp_1", "amp_2", "amp_3")] == [40, 48, 3] and len(unlisted) == 6
    lines = ["single\tamp_1", ""]                                   # (replaced below: the last line of a read id counts)
    for primer in ("amp_1", "amp_2", "amp_3"):
        lines += ["%s\t%s" % (name, primer) for name, _ in named[primer]]
    lines += ["", "not_in_the_sample\tamp_empty"]
    D = Dealt()
    D.table = "\n".join(lines) + "\n"
    D.group_names, of_read = parse_table(D.table)
    everything = named["amp_1"] + named["amp_2"] + named["amp_3"] + unlisted
    order = np.random.default_rng(1216).permutation(len(everything))
    D.names = [everything[i][0] for i in order]
    D.reads = [everything[i][1] for i in order]
    D.groups = groups_of(D.names, len(D.group_names), of_read)
    D.long = D.names.index("long")
    return D


@functools.lru_cache(maxsize=None)
def family_merged():
    D = family()
    return merge_by_group(D.reads, D.groups, len(D.group_names))


@functools.lru_cache(maxsize=None)
def truncation_set():
    """a group of exactly 100 raw reads -- 29 copies of one read, 28 of another, 43 of a third, no k-min-mer in common -- and
    one unlisted read: 0.29 x 100 is 28.999... as a double and truncates to 28, so the 28 copies go and the 29 stay"""
    iso = mc.family().isolated
    D = Dealt()
    D.reads = [iso[0]] * 29 + [iso[1]] * 28 + [iso[2]] * 43 + [iso[3]]
    D.names = ["big%03d" % i for i in range(100)] + ["alone"]
    D.table = "".join("%s\tbig\n" % x for x in D.names[:100])
    D.group_names, of_read = parse_table(D.table)
    D.groups = groups_of(D.names, 1, of_read)
    return D


# (mask_reads, mask_seeds, reads_rf, seeds_rf) of the exact comparisons on the device: groups alone, the absolute masks, the relative ones
SETTINGS = ((0, 0, 0.0, 0.0), (1, 0, 0.0, 0.0), (0, 2, 0.0, 0.0), (0, 0, 0.05, 0.0), (0, 0, 0.0, 0.05))
