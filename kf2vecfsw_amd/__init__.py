"""kf2vecfsw_amd -- MI355X-native replacement of kf2vec's k-mer frequency-vector
builder (`get_frequencies`, reference kf2vec/main.py:250-373).

Layout:
  csrc/kf_count.hip   HIP kernels (gfx950) + device half of the C-ABI
  csrc/kf_host.cpp    host half of the C-ABI (tables, record index, .kf writer)
  _native.py          ctypes binding of libkf2vec_gpu.so (no CPU fallback)
  counter.py          batch packing + KmerCounter (device counting)
  main.py             `get_frequencies` CLI mirror
  features.py         a get_frequencies `.kf` directory as the trainers' float64 matrix
  tables.py           distance matrices and embedding tables (tab-separated floats) on the device: read
                      (kf_parse_tsv_floats) and written (kf_format_float_rows, write_float_table)
  query.py            `query`: distances to a clade's backbone (kf_sq_distances) and embeddings, written
                      as text formatted on the device
  classify.py         `classify`: the classifier's forward pass, kf_class_probs (softmax in the direct form,
                      first-index argmax, the classes.out row) and classes.out written from the device;
                      main.py's `process_query_data` runs get_frequencies, classify and query in turn
  train.py            `train_model_set`: the distance model of every clade, a step's loss and gradient in
                      one call (kf_dist_loss)
  train_classifier.py `train_classifier`: the clade classifier, a step's loss, gradient, right classes and
                      the epoch's totals in one call (kf_class_loss); writes classifier_model.ckpt and
                      backbone_classes.out
"""
__all__ = ["__version__"]
__version__ = "0.1.0"
