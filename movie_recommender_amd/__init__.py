"""MI355X-native ALS core for louisyang2015/movie_recommender.

Hot path: the per-user / per-movie least-squares half-steps of ALS training
(reference ``cpp/ls_lib/matrix.cpp:744-1031``) as hand-written HIP kernels for
gfx950, behind the reference's ctypes ABI (``cpp_ls_lib.so``).

Modules
  cpp_ls      drop-in for the reference ``cpp/python/cpp_ls.py``
  engine      device-resident ALS context (``include/mr_als.h``)
  implicit    implicit-feedback (confidence-weighted) ALS on the same context
  foldin      new users / items for every model kind (``include/mr_foldin.h``)
  content     tag least-squares content model (``include/mr_content.h``)
  tagcount    tag-count content model, median predictor (``include/mr_tagcount.h``)
  lsqr        general sparse LSQR and the SciPy-style ALS on it (``include/mr_lsqr.h``)
  lsmr        SciPy's LSMR on the same resident matrix, and the ALS with it
  svds        SciPy's svds (k largest singular triplets) on the same resident matrix
  puresvd     PureSVD: the rating matrix's truncated SVD as a served factor model
  distributed one process per GPU, users/items sharded, factor all-gather
  synth       seeded MovieLens-shaped ratings (benchmarks, statistical tests)
  build       compiles ``lib/cpp_ls_lib.so`` with hipcc for gfx950
"""
__version__ = "0.1.0"
