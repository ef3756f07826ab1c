"""The device tables of groot_hip_open as plain host functions (groot_amd/csrc/hip/index_tables.hpp), on a CPU: tools/open_tables_check.cpp is
compiled with the host library's sources under AddressSanitizer + UBSan and run as a child process.  It builds an index from test.gfa,
test2.gfa, test-genes.msa and the first 24 clusters of arg-annot.90 and two hand-made views, runs every builder on each, checks what can be
checked without a device (every window is in the exact table, every band's ids are a permutation sorted by its keys, bases2 decodes back
to every ACGT base, a path's text is the concatenation of its nodes, the 2^31 guard at its edge) and prints size and FNV-1a of every table.

Where the pins below come from: the lines of the four fixture indices are what the PARENT of the commit that introduced index_tables.hpp
uploaded -- its upload() printed byte count and FNV-1a of every source buffer while a ctx was opened on an MI355X for each index
(profiles/r19_open_unit.txt), and every pinned (bytes, hash) of a table that does not depend on the device was found in that sequence.
Lines that have no parent value, pinned from index_tables.hpp itself: node_graph and sketch_class (host-only vectors, never uploaded),
`sig` (argmin and verdicts come from the device at open; the program passes none), the path_texts / band_hash_bits / bit_addressable32
lines (no table), text / tlen / win_nodes of the two .gfa indices (sketch size 10: no signature index, a ctx never builds them), and both hand-made views.  What protects those is the
sanitizer run and the program's own checks."""
import os
import subprocess
import tarfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(REPO, "tests", "golden", "data")
HOST_SRC = ["index.cpp", "gob.cpp", "graphs.cpp", "fastq.cpp", "reads.cpp", "bam.cpp", "report.cpp"]

PINS = """\
bit_addressable32  2147483135  1
bit_addressable32  2147483136  0
bit_addressable32  4294967296  0
test.gfa/node_rec  8512  9445edaacb348633
test.gfa/node_graph  532  b92f1b94797eb135
test.gfa/path_node  4256  35e3e9464171e801
test.gfa/path_text  1200  604a27960ee313b3
test.gfa/path_tag  1200  5d76ac2ad2217464
test.gfa/path_nodes  2108  53b1765be6421ebf
test.gfa/path_tab  88536  7a6cd36261157a3f
test.gfa/path_texts  6 of 6 paths, 4484 bases
test.gfa/bases2  280  754eec77b59019e3
test.gfa/lean_nodes  8512  bc40296ce8d81309
test.gfa/lean_ext  8512  5dc947a2a2257d00
test.gfa/cn_pre2  86768  701a958b9326872a
test.gfa/win_ok  965  74b46dc8466a1a88
test.gfa/cn_pre  173536  c623be8f7bfd9759
test.gfa/node_l2b  11704  2e887d4fadff49de
test.gfa/graph_win_end  4  433d9196a5c6cde1
test.gfa/graph_words  1  af63bc4c8601b62c
test.gfa/win_rec  30880  79acdca499d978a9
test.gfa/exact  16384  5b98c2cff9bce700
test.gfa/sketch_class  3860  c9d2dc78d2aafc72
test.gfa/band_keys  30880  c94ec6f2caa2ebb2
test.gfa/band_ids  7720  280131d8ab8ef071
test.gfa/band_hash  131072  0555140da2513d6d
test.gfa/band_sig  30880  f488f20a721b71ad
test.gfa/band_run  30880  e5f070daeb88b45c
test.gfa/band_hash_bits  11
test.gfa/q_k  251  7b90ff945cb75ea1
test.gfa/q_l  251  f9fb43540aa61899
test.gfa/q_min_eq  502  e19f0909c3a77c66
test.gfa/text  494144  54930a41fb03b34c
test.gfa/tlen  3860  4b5971dd64ef94bc
test.gfa/win_nodes  965  536de68cd4a5713d
test2.gfa/node_rec  15360  cea1433c0430515f
test2.gfa/node_graph  960  c42a06f7e7a28e25
test2.gfa/path_node  7680  29fb2b2b11bdf8c5
test2.gfa/path_text  492  6abfd53ea3d71495
test2.gfa/path_tag  492  87c1ab525fa7656a
test2.gfa/path_nodes  1632  1087d76ed3564439
test2.gfa/path_tab  78336  e53f95adbbcb9465
test2.gfa/path_texts  2 of 2 paths, 1650 bases
test2.gfa/bases2  296  5d16ac3e5c0f98f0
test2.gfa/lean_nodes  15360  4cb4288fa0bebb5f
test2.gfa/lean_ext  15360  b49ec45e8f331e31
test2.gfa/cn_pre2  67344  5ed05c9b6f122790
test2.gfa/win_ok  487  30212366aae96e1e
test2.gfa/cn_pre  134688  da609149f1932a05
test2.gfa/node_l2b  21120  f47a5939d2644971
test2.gfa/graph_win_end  4  728a729c81aab78d
test2.gfa/graph_words  1  af63bc4c8601b62c
test2.gfa/win_rec  15584  951078aad3b81a9d
test2.gfa/exact  8192  bc92a7eecf2edaaf
test2.gfa/sketch_class  1948  63a41c95e9205725
test2.gfa/band_keys  15584  f16ddeac4e876df0
test2.gfa/band_ids  3896  9984ca821655e791
test2.gfa/band_hash  65536  e8827df3ccf48c3c
test2.gfa/band_sig  15584  00ffe67b8ce87bed
test2.gfa/band_run  15584  c2702d00bc54959e
test2.gfa/band_hash_bits  10
test2.gfa/q_k  251  7b90ff945cb75ea1
test2.gfa/q_l  251  f9fb43540aa61899
test2.gfa/q_min_eq  502  e19f0909c3a77c66
test2.gfa/text  249408  4471975a303f2126
test2.gfa/tlen  1948  66594d595d6c5d36
test2.gfa/win_nodes  487  d0021ad781cef415
test-genes.msa/node_rec  20416  9562277b9a468c4a
test-genes.msa/node_graph  1276  cc9f372d25953b55
test-genes.msa/path_node  10208  317ef654baa08302
test-genes.msa/path_text  16772  2c5c89cd43a58242
test-genes.msa/path_tag  16772  9ca78af321acdc2b
test-genes.msa/path_nodes  66216  03bce9e4606bb3c0
test-genes.msa/path_tab  3178368  80645b7d63252184
test-genes.msa/path_texts  81 of 81 paths, 66774 bases
test-genes.msa/bases2  316  2895af3fcfd8bfa8
test-genes.msa/lean_nodes  20416  d9780236b23bc849
test-genes.msa/lean_ext  20416  defabda290df8d31
test-genes.msa/cn_pre2  3500336  dd762f27c048092f
test-genes.msa/win_ok  8405  07135cb4a9108378
test-genes.msa/cn_pre  7000672  9f0529dced9c8eba
test-genes.msa/node_l2b  28072  9b7e31e3e7f90b12
test-genes.msa/graph_win_end  4  3e1b411c976a7050
test-genes.msa/graph_words  1  af63c64c8601c72a
test-genes.msa/win_rec  268960  b7ebd7e3cded24e8
test-genes.msa/exact  262144  fe62f74062a9a908
test-genes.msa/sketch_class  33620  bda88575c5b0bc77
test-genes.msa/band_keys  941360  c1bf8a3f031556e5
test-genes.msa/band_ids  235340  8de39ca6530cc3c5
test-genes.msa/band_hash  7340032  87a3bf86b31b770d
test-genes.msa/band_sig  941360  2ac5853a1574ec19
test-genes.msa/band_run  941360  9fc6145a1bf85e5e
test-genes.msa/band_hash_bits  15
test-genes.msa/q_k  207  2d3651545b80572b
test-genes.msa/q_l  207  e63bc38eabe32d5d
test-genes.msa/q_min_eq  414  cc18c90953e6f44e
test-genes.msa/text  4303424  41874ccbb64a679c
test-genes.msa/tlen  33620  1b18447efc5d112b
test-genes.msa/win_nodes  8405  b3d1093c9c735bef
test-genes.msa/sig  269216  3fae9bb1c1868239
test-genes.msa/sig_dir  262144  5484e28a6870973f
arg-annot.90[:24]/node_rec  16640  5bd8cadb1b2d9fea
arg-annot.90[:24]/node_graph  1040  cbdad1fd1e3cf459
arg-annot.90[:24]/path_node  8320  e332a8a79f70b342
arg-annot.90[:24]/path_text  5512  5f9dae5cefccd941
arg-annot.90[:24]/path_tag  5512  3645ff2b683900ff
arg-annot.90[:24]/path_nodes  1956  43e951799940bac2
arg-annot.90[:24]/path_tab  75096  ead48b06dbd63c07
arg-annot.90[:24]/path_texts  29 of 29 paths, 21729 bases
arg-annot.90[:24]/bases2  4516  47c97bfd2501cbaa
arg-annot.90[:24]/lean_nodes  16640  6da127b7df418dbb
arg-annot.90[:24]/lean_ext  16640  8b087285268a7bf4
arg-annot.90[:24]/cn_pre2  373328  28bc939b04de5a3d
arg-annot.90[:24]/win_ok  8206  6cae4c9bf5dc92f3
arg-annot.90[:24]/cn_pre  746656  e0227bd3477622b6
arg-annot.90[:24]/node_l2b  22880  0189936fc4b2efdf
arg-annot.90[:24]/graph_win_end  96  b4bf9ddb7e9cb737
arg-annot.90[:24]/graph_words  24  43b103a307f3ee9d
arg-annot.90[:24]/win_rec  262592  94a907b4b0466066
arg-annot.90[:24]/exact  262144  1c36a31b16436ffd
arg-annot.90[:24]/sketch_class  32824  d35fffef93a98da8
arg-annot.90[:24]/band_keys  656480  dd42340e70f55e1b
arg-annot.90[:24]/band_ids  164120  80185794ad2cd4b4
arg-annot.90[:24]/band_hash  5242880  a4d5c4afef11d130
arg-annot.90[:24]/band_sig  656480  fafad4fd44f70da4
arg-annot.90[:24]/band_run  656480  71fb0a1aba08ec5d
arg-annot.90[:24]/band_hash_bits  15
arg-annot.90[:24]/q_k  227  521d93163c54bb2b
arg-annot.90[:24]/q_l  227  a5c90b30eab7a6a1
arg-annot.90[:24]/q_min_eq  454  51ad56d18154ef08
arg-annot.90[:24]/text  4201536  4de3bef4eca1ec37
arg-annot.90[:24]/tlen  32824  f4ba53f408dcc2fb
arg-annot.90[:24]/win_nodes  8206  2edcef2e81a92da3
arg-annot.90[:24]/sig  262848  e1d600df652407ac
arg-annot.90[:24]/sig_dir  262144  9066235384f0be7e
hand-made/node_rec  576  44be9da2303a626e
hand-made/node_graph  36  153cd7878c89c0e5
hand-made/path_node  288  f8a5c28603779202
hand-made/path_text  96  7060b6ec18595242
hand-made/path_tag  96  f14aa9973dddc703
hand-made/path_nodes  44  27e624d7171f987b
hand-made/path_tab  528  86807e4ad944ec03
hand-made/path_texts  4 of 5 paths, 73 bases
hand-made/bases2  96  47fed6990d227fb0
hand-made/lean_nodes  576  d3e6aa08e2fb8f86
hand-made/lean_ext  576  b9d0059d61083025
hand-made/cn_pre2  176  806d08588ceb287f
hand-made/win_ok  6  cf3ee6fa24b85408
hand-made/cn_pre  352  5f301ce28ee978de
hand-made/node_l2b  792  f07e9ac75d066bbb
hand-made/graph_win_end  8  ecbce440019f7ca7
hand-made/graph_words  2  082f2307b4e88e77
hand-made/win_rec  192  c41caa972f79aed5
hand-made/exact  128  da3d7ef6d34ad00e
hand-made/sketch_class  24  4c5dbfe1d07a6bc5
hand-made/band_keys  384  831edac953dcce8e
hand-made/band_ids  96  b94d2802aeec5fb5
hand-made/band_hash  2048  9a2342cbc594a335
hand-made/band_sig  384  97772a849d769fc5
hand-made/band_run  384  d1a036db829bb5a5
hand-made/band_hash_bits  4
hand-made/q_k  255  3c01c63727bb6c99
hand-made/q_l  255  ab89d5d22e80ab4d
hand-made/q_min_eq  510  7c5eca05eeaab4cc
hand-made/text  3136  5251c328f6bd9962
hand-made/tlen  24  d9a97c4f6deb71e2
hand-made/win_nodes  6  e60d650b93b1ea8d
hand-made/sig  448  6afa879b6836b6c8
hand-made/sig_dir  256  8f10e28bbaa848af
hand-made, no windows/node_rec  576  44be9da2303a626e
hand-made, no windows/node_graph  36  153cd7878c89c0e5
hand-made, no windows/path_node  288  f8a5c28603779202
hand-made, no windows/path_text  96  7060b6ec18595242
hand-made, no windows/path_tag  96  f14aa9973dddc703
hand-made, no windows/path_nodes  44  27e624d7171f987b
hand-made, no windows/path_tab  528  86807e4ad944ec03
hand-made, no windows/path_texts  4 of 5 paths, 73 bases
hand-made, no windows/bases2  96  47fed6990d227fb0
hand-made, no windows/lean_nodes  576  d3e6aa08e2fb8f86
hand-made, no windows/lean_ext  576  b9d0059d61083025
hand-made, no windows/cn_pre2  16  88201fb960ff6465
hand-made, no windows/win_ok  0  cbf29ce484222325
hand-made, no windows/cn_pre  32  0c8210784d8af5a5
hand-made, no windows/node_l2b  792  f07e9ac75d066bbb
hand-made, no windows/graph_win_end  8  a8c7f832281a39c5
hand-made, no windows/graph_words  2  082f2307b4e88e77
hand-made, no windows/win_rec  0  cbf29ce484222325
hand-made, no windows/exact  128  8ea7cd390263cce5
hand-made, no windows/sketch_class  0  cbf29ce484222325
hand-made, no windows/band_keys  0  cbf29ce484222325
hand-made, no windows/band_ids  0  cbf29ce484222325
hand-made, no windows/band_hash  2048  175cb070add98725
hand-made, no windows/band_sig  0  cbf29ce484222325
hand-made, no windows/band_run  0  cbf29ce484222325
hand-made, no windows/band_hash_bits  4
hand-made, no windows/q_k  255  3c01c63727bb6c99
hand-made, no windows/q_l  255  ab89d5d22e80ab4d
hand-made, no windows/q_min_eq  510  7c5eca05eeaab4cc
ok
"""


def test_every_table_builder_under_sanitizers(tmp_path):
    flags = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
             "-I" + os.path.join(REPO, "include"), "-I" + os.path.join(REPO, "groot_amd", "csrc", "hip")]
    src = [os.path.join(REPO, "tools", "open_tables_check.cpp")] + [os.path.join(REPO, "groot_amd", "csrc", "host", f) for f in HOST_SRC]
    objs = [str(tmp_path / (os.path.basename(s) + ".o")) for s in src]
    jobs = [subprocess.Popen(flags + ["-c", s, "-o", o], stderr=subprocess.PIPE, text=True) for s, o in zip(src, objs)]   # (side by side: two minutes one after the other)
    for s, j in zip(src, jobs):
        err = j.communicate()[1]
        assert j.returncode == 0, (s, err[-3000:])
    exe = str(tmp_path / "open_tables_check")
    subprocess.run(flags + ["-o", exe] + objs + ["-lpthread", "-lz"], check=True)
    with tarfile.open(os.path.join(DATA, "arg-annot.90.tar.gz")) as tf:
        names = sorted(n for n in tf.getnames() if os.path.basename(n).startswith("cluster") and n.endswith(".msa"))[:24]
        tf.extractall(tmp_path, members=[tf.getmember(n) for n in names])
    args = [os.path.join(DATA, f) for f in ("test.gfa", "test2.gfa", "test-genes.msa")] + [str(tmp_path / n) for n in names]
    r = subprocess.run([exe] + args, capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", (r.stdout[-2000:], r.stderr[-3000:])
    got, want = r.stdout.splitlines(), PINS.splitlines()
    assert got[-1] == "ok"
    for g, w in zip(got, want):
        assert g == w, (g, w)
    assert len(got) == len(want)
