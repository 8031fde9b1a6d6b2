"""Genotype + consensus stages (pmx_pileup_* / pmx_genotype_*; runGenotyping / runConsensus, src/main.cpp:1828-1900).
ctypes mirror only: `Pileup` runs the device pileup over an Aligner's resident results (or over fetched records) and
returns the integer tables, `Genotyper` turns tables into VCF records and writes `<prefix>.vcf` / `<prefix>.consensus.fa`."""
import ctypes as C

import numpy as np

from ._lib import lib, check, PmxError
from .api import Aligner, Context, Panman, ReadSet

HIST = 640   # PMX_PILEUP_HIST: [q 0..63][strand][A C G T N]
AUX = 4      # PMX_PILEUP_AUX: raw depth, sum of capped mapQ, bases of MQ-0 reads, deletions
HIST_SHAPE = (64, 2, 5)
BIAS = 760   # PMX_PILEUP_BIAS: pos [2][100], scl [2][100], mq [2][60], bq [2][60] by ref/alt, mqs [2][60] by strand
BIAS_BLOCKS = dict(pos=(0, 100), scl=(200, 100), mq=(400, 60), bq=(520, 60), mqs=(640, 60))   # PMX_PLB_*: offset, bins
TEST_KEYS = ("VDB", "SGB", "RPBZ", "MQBZ", "MQSBZ", "BQBZ", "SCBZ", "MQ0F")

ADMITTED, RECONCILED, SECOND_MATE, KEEPS_AGREEING = 1, 2, 4, 8   # bits of Pileup.read_info()[0]


class PileupParams(C.Structure):
    """pmx_pileup_params (defaults: src/3rdparty/bcftools/mpileup.c:1363-1367, bam2bcf.c:49)"""
    _fields_ = [("max_depth", C.c_int32), ("min_baseq", C.c_int32), ("max_baseq", C.c_int32), ("delta_baseq", C.c_int32),
                ("cap_mapq", C.c_int32), ("reserved", C.c_int32 * 3)]

    def __init__(self, max_depth=250, min_baseq=1, max_baseq=60, delta_baseq=30, cap_mapq=60):
        super().__init__(max_depth, min_baseq, max_baseq, delta_baseq, cap_mapq)


class SiteCall(C.Structure):
    """pmx_site_call"""
    _fields_ = [("n_alleles", C.c_int32), ("alleles", C.c_int32 * 5), ("pl", C.c_int32 * 5), ("ad", C.c_int32 * 5), ("dp4", C.c_int32 * 4),
                ("n_bases", C.c_int32), ("reserved", C.c_int32 * 3)]


class SiteTests(C.Structure):
    """pmx_site_tests"""
    _fields_ = [("value", C.c_float * 8), ("present", C.c_uint32), ("reserved", C.c_uint32 * 3)]


def _names(names):
    """list of bytes -> (concat buffer, offsets) as pmx_pileup_run takes them; None stays None"""
    if names is None:
        return None, None
    off = np.zeros(len(names) + 1, np.int64)
    off[1:] = np.cumsum([len(x) for x in names])
    return C.create_string_buffer(b"".join(names), int(off[-1]) + 1), off


class Pileup:
    def __init__(self, ctx: Context):
        self.ctx = ctx
        self._h = C.c_void_p()
        self.ref_len = 0
        self.n_reads = 0
        check(lib.pmx_pileup_create(ctx._h, C.byref(self._h)), "pmx_pileup_create")

    def run(self, aligner: Aligner, rs: ReadSet, ref_len: int, paired: bool, revcomp_mate2: bool = False, names=None, params: PileupParams = None):
        """the pileup of the aligner's last align_readset(rs, ...) -- records, CIGARs and reads stay on the device"""
        nb, noff = _names(names)
        pp = params or PileupParams()
        check(lib.pmx_pileup_run(self.ctx._h, self._h, aligner._h, rs._h, int(ref_len), int(paired), int(revcomp_mate2),
                                 C.addressof(nb) if nb is not None else None, noff.ctypes.data if noff is not None else None, C.addressof(pp)),
              "pmx_pileup_run")
        self.ref_len, self.n_reads = int(ref_len), rs.n_reads

    def run_records(self, recs, cigars, concat, offsets, ref_len: int, paired: bool, revcomp_mate2: bool = False, quals=None, names=None,
                    params: PileupParams = None):
        """the same from fetched records (Aligner.fetch / Dist.fetch_gathered) and host reads"""
        recs = np.ascontiguousarray(recs)
        cigars = np.ascontiguousarray(cigars, np.uint32)
        concat = np.ascontiguousarray(np.frombuffer(concat, np.uint8) if isinstance(concat, (bytes, bytearray)) else concat, np.uint8)
        offsets = np.ascontiguousarray(offsets, np.int64)
        q = None if quals is None else np.ascontiguousarray(np.frombuffer(quals, np.uint8) if isinstance(quals, (bytes, bytearray)) else quals, np.uint8)
        nb, noff = _names(names)
        pp = params or PileupParams()
        check(lib.pmx_pileup_run_records(self.ctx._h, self._h, recs.ctypes.data, len(recs), cigars.ctypes.data, len(cigars), concat.ctypes.data,
                                         q.ctypes.data if q is not None else None, offsets.ctypes.data, int(ref_len), int(paired), int(revcomp_mate2),
                                         C.addressof(nb) if nb is not None else None, noff.ctypes.data if noff is not None else None, C.addressof(pp)),
              "pmx_pileup_run_records")
        self.ref_len, self.n_reads = int(ref_len), len(recs)

    def tables(self):
        """-> (hist uint32 [ref_len, 64, 2, 5], aux uint32 [ref_len, 4])"""
        hist = np.zeros((self.ref_len,) + HIST_SHAPE, np.uint32)
        aux = np.zeros((self.ref_len, AUX), np.uint32)
        check(lib.pmx_pileup_fetch(self.ctx._h, self._h, hist.ctypes.data, aux.ctypes.data), "pmx_pileup_fetch")
        return hist, aux

    def bias(self, positions, ref_bases: bytes):
        """the bias pass of the last run at the listed sites (0-based, strictly ascending; one reference letter each)
        -> uint32 [n, 760], blocks as BIAS_BLOCKS"""
        positions = np.ascontiguousarray(positions, np.int32)
        ref_bases = bytes(ref_bases)
        if positions.ndim != 1 or len(ref_bases) != len(positions):
            raise ValueError("bias: one reference letter per position")
        out = np.zeros((len(positions), BIAS), np.uint32)
        check(lib.pmx_pileup_bias(self.ctx._h, self._h, positions.ctypes.data, ref_bases, len(positions), out.ctypes.data), "pmx_pileup_bias")
        return out

    def read_info(self):
        """-> (flags uint8 per read: ADMITTED | RECONCILED | SECOND_MATE | KEEPS_AGREEING, rank in the BAM uint32 per read)"""
        flags = np.zeros(max(self.n_reads, 1), np.uint8)
        rank = np.zeros(max(self.n_reads, 1), np.uint32)
        check(lib.pmx_pileup_read_info(self._h, flags.ctypes.data, rank.ctypes.data, len(flags)), "pmx_pileup_read_info")
        return flags[:self.n_reads], rank[:self.n_reads]

    def bytes_moved(self) -> int:
        return int(lib.pmx_pileup_bytes(self._h))

    def close(self):
        if self._h:
            lib.pmx_pileup_free(self.ctx._h, self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def spectrum_counts(pm: Panman):
    """-> (counts int64 [4, 4] from -> to, branches, genome length of the ten DFS-spaced leaves' median)"""
    counts = np.zeros(16, np.int64)
    nb, gl = C.c_int64(0), C.c_int64(0)
    check(lib.pmx_genotype_spectrum_counts(pm._h, counts.ctypes.data, C.byref(nb), C.byref(gl)), "pmx_genotype_spectrum_counts")
    return counts.reshape(4, 4), int(nb.value), int(gl.value)


def spectrum_phred(counts, branches: int, genome_len: int):
    """-> phred float64 [4, 4], or None when the tree shows no substitution (the reference then runs without a spectrum)"""
    counts = np.ascontiguousarray(np.asarray(counts, np.int64).reshape(16))
    out = np.zeros(16, np.float64)
    rc = lib.pmx_genotype_spectrum_phred(counts.ctypes.data, int(branches), int(genome_len), out.ctypes.data)
    if rc < 0:
        raise PmxError(rc, "pmx_genotype_spectrum_phred")
    return None if rc == 1 else out.reshape(4, 4)


def site_call(hist, ref_base: bytes) -> dict:
    """one site from its hist[pos]: alleles (0..4 = A C G T N, reference first), haploid PL, AD, DP4"""
    h = np.ascontiguousarray(np.asarray(hist, np.uint32).reshape(HIST))
    sc = SiteCall()
    check(lib.pmx_genotype_site(h.ctypes.data, ref_base[:1], C.byref(sc)), "pmx_genotype_site")
    n = sc.n_alleles
    return dict(alleles=list(sc.alleles[:n]), pl=list(sc.pl[:n]), ad=list(sc.ad[:n]), dp4=list(sc.dp4), n_bases=sc.n_bases)


def format_float(v) -> str:
    """a float as a VCF prints it (htslib's kputd)"""
    buf = C.create_string_buffer(64)
    lib.pmx_genotype_format_float(float(v), buf, len(buf))
    return buf.value.decode()


def site_tests(hist_row, aux_row, bias_row, ref_base: bytes) -> dict:
    """mpileup's bias annotations of one site -> {key: value as the VCF prints it}, absent keys left out (TEST_KEYS order)"""
    h = np.ascontiguousarray(np.asarray(hist_row, np.uint32).reshape(HIST))
    a = np.ascontiguousarray(np.asarray(aux_row, np.uint32).reshape(AUX))
    b = np.ascontiguousarray(np.asarray(bias_row, np.uint32).reshape(BIAS))
    t = SiteTests()
    check(lib.pmx_genotype_site_tests(h.ctypes.data, a.ctypes.data, b.ctypes.data, ref_base[:1], C.byref(t)), "pmx_genotype_site_tests")
    return {lib.pmx_genotype_test_name(k).decode(): format_float(t.value[k]) for k in range(len(TEST_KEYS)) if t.present >> k & 1}


def filter_line(line: str, phred=None, min_depth: int = 1, min_qual: float = 30.0) -> str:
    """applyMutationSpectrum on one VCF line (phred None: the branch without a spectrum); '' = dropped"""
    p = None if phred is None else np.ascontiguousarray(np.asarray(phred, np.float64).reshape(16))
    buf = C.create_string_buffer(len(line) + 256)
    n = lib.pmx_genotype_filter_line(line.encode(), p.ctypes.data if p is not None else None, int(min_depth), float(min_qual), buf, len(buf))
    if n < 0:
        raise PmxError(int(n), "pmx_genotype_filter_line")
    return buf.value.decode()


class Genotyper:
    """calls of one genome from the pileup tables"""

    def __init__(self, hist, aux, reference: bytes, chrom: str, phred=None, min_depth: int = 1, min_qual: float = 30.0):
        hist = np.ascontiguousarray(hist, np.uint32)
        aux = np.ascontiguousarray(aux, np.uint32)
        p = None if phred is None else np.ascontiguousarray(np.asarray(phred, np.float64).reshape(16))
        self._h = C.c_void_p()
        self.chrom, self.ref_len = chrom, len(reference)
        n = lib.pmx_genotype_call(hist.ctypes.data, aux.ctypes.data, bytes(reference), len(reference), chrom.encode(),
                                  p.ctypes.data if p is not None else None, int(min_depth), float(min_qual), C.byref(self._h))
        if n < 0:
            raise PmxError(int(n), "pmx_genotype_call")

    def records(self):
        return [lib.pmx_genotype_record(self._h, i).decode() for i in range(lib.pmx_genotype_num_records(self._h))]

    def positions(self):
        """0-based reference position of every record"""
        return np.asarray([lib.pmx_genotype_record_pos(self._h, i) for i in range(lib.pmx_genotype_num_records(self._h))], np.int32)

    def annotate(self, positions, bias):
        """adds mpileup's bias annotations to the INFO of the records at `positions` (bias: Pileup.bias at those positions)"""
        positions = np.ascontiguousarray(positions, np.int32)
        bias = np.ascontiguousarray(bias, np.uint32)
        if bias.size != len(positions) * BIAS:
            raise ValueError("annotate: one bias row per position")
        check(lib.pmx_genotype_annotate(self._h, positions.ctypes.data, bias.ctypes.data, len(positions)), "pmx_genotype_annotate")

    def write_vcf(self, path: str, sample_name: str):
        check(lib.pmx_genotype_write_vcf(self._h, path.encode(), self.chrom.encode(), self.ref_len, sample_name.encode()), "pmx_genotype_write_vcf")

    def close(self):
        if self._h:
            lib.pmx_genotype_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def write_consensus(vcf_path: str, ref_fa_path: str, out_path: str, header: str):
    check(lib.pmx_genotype_write_consensus(vcf_path.encode(), ref_fa_path.encode(), out_path.encode(), header.encode()), "pmx_genotype_write_consensus")
