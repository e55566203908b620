"""Crafted FASTQ inputs shared by the piece-wise path's CPU and GPU tests."""
import gen


def fastq_reads(rng, n, length=None, qual_first=b"", crlf=False, name=b"r"):
    """n four-line records; qual_first: the bytes a quality line may start with."""
    nl = b"\r\n" if crlf else b"\n"
    out = []
    for i in range(n):
        L = int(rng.integers(1, 200)) if length is None else length
        seq = gen.random_seq(rng, L, n_rate=0.01).tobytes()
        q = bytearray(rng.choice(list(b"ACGT!#II@+~"), size=L).tolist())
        if qual_first:
            q[0] = qual_first[i % len(qual_first)]
        out.append(b"@" + name + b"%d x" % i + nl + seq + nl + (b"+" if i % 2 else b"+" + name + b"%d" % i) + nl
                   + bytes(q) + nl)
    return b"".join(out)
