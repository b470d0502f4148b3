"""The names the steps' shared plumbing has always been reached by (bench.py, run_sample.py, tools/): a facade.  Where they live:
    irn_amd/_tuned.py   device key, shipped MIOpen databases and GEMM tables, MIOpen set-up, the reproducible mode
    step/_pool.py       ModelSpec, worker devices, the persistent worker pool, spawn_workers
    step/_stores.py     CamStore / EdgeStore and their run stamps, CAM-owner aware shards
    step/_io.py         loader threads, page-locked pool, uploads, writer threads, shard_io
    step/_report.py     start-up and summary lines, the fp16-range check, the counters bench.py reads
    step/_labels.py     walk_radius, make_walker
    step/_split_auto.py `--split_gemm auto`: per-image fp16-range flags on their way to the host, the redo list
Every object has one home, is only ever changed in place and is never rebound, so `_common.CAM_STORE` IS `_stores.CAM_STORE`.
Code inside the package imports the home modules, and that is where it looks names up: a monkeypatch has to name the home
module, a patch of `_common` reaches nobody."""
# (modules and classes the one-file version imported at its top, and thereby exposed)
import atexit                                                                              # noqa: F401
import importlib                                                                           # noqa: F401
import os                                                                                  # noqa: F401
import pickle                                                                              # noqa: F401
import traceback                                                                           # noqa: F401
from concurrent.futures import ThreadPoolExecutor                                          # noqa: F401
from multiprocessing.reduction import ForkingPickler                                       # noqa: F401

import numpy as np                                                                         # noqa: F401
import torch                                                                               # noqa: F401
from torch import multiprocessing                                                          # noqa: F401
from torch.utils.data import Subset                                                        # noqa: F401

from .._tuned import (_MIOPEN_LOCKS, _WARNED, apply_deterministic_setting, deterministic_backbones, gemm_table_root,   # noqa: F401
                      merge_miopen_db, miopen_cache_key, miopen_mode_key, miopen_seed_root, miopen_setup,
                      reap_private_miopen_dbs, shipped_data_report, warn_missing_shipped_data)
from ._io import (_UPLOADS, MAX_LOADER_THREADS, PINNED, AsyncWriter, PinnedPool, device_images, device_preprocess,       # noqa: F401
                  make_loader, progress, set_skip_image, upload, writer_threads)
from ._labels import make_walker, walk_radius                                                                           # noqa: F401
from ._pool import (_MODELS, _POOL, ModelSpec, WorkerPool, get_pool, import_network, materialise, n_gpus_or_raise,       # noqa: F401
                    pool_stats, shutdown_workers, spawn_workers, step_timeout, worker_device, worker_devices)
from ._report import (CAM_STATS, SPLIT_STATS, WALK_STATS, check_split_overflow, say, startup_line, step_summary,                     # noqa: F401
                      untuned_report)
from ._stores import (CAM_OWNERS, CAM_STORE, EDGE_STORE, CamStore, EdgeStore, current_cam_run, image_stamp,              # noqa: F401
                      keep_cams, keep_edges, label_step_shards, new_cam_run, split_by_owner)
