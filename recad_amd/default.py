"""Default configuration registry for the victim path.

Mirrors the keys and values of the reference's registry for the three victims, the random, average, segment, bandwagon, AUSH, AIA, AushPlus and UBA attackers,
the PCASelectUsers defender (recad/default.py:103-221,223-228) and the implicit / explicit dataset and workflow knobs the
hot path reads (recad/default.py:49-99,247-267).  Only what the path needs is present.  Entries marked build-specific (the
later victims and defenders, the PGA attacker) have no counterpart there.
"""
import logging
import os

import torch

SEED = 2023  # recad/default.py:21
DEVICE = torch.device("cuda" if torch.cuda.is_available() else "cpu")

MODEL = {
    "victim": {
        "lightgcn": {
            "latent_dim_rec": 128, "lightGCN_n_layers": 3, "A_split": False, "pretrain": False, "keep_prob": 0.6,
            "dropout": 0.0, "lambda": 1e-4, "optim": "adam", "lr": 1e-3,
        },
        "mf": {"factor_num": 3, "embedding_size": 128, "dropout": 0, "optim": "adam", "lr": 1e-3},
        "ncf": {
            "factor_num": 32, "num_layers": 5, "dropout": 0, "model": "NeuMF-end", "GMF_model": None, "MLP_model": None,
            "optim": "adam", "lr": 1e-3,
        },
        # build-specific (no reference counterpart): item-neighbourhood CF, victim/itemknn.py; band / user_block None = automatic
        "itemknn": {"k": 50, "band": None, "user_block": None},
        # build-specific (no reference counterpart): the closed-form item-item autoencoder (Steck 2019), victim/ease.py;
        # block None = automatic
        "ease": {"reg_lambda": 500.0, "block": None},
        # build-specific (no reference counterpart): implicit-feedback ALS (Hu, Koren and Volinsky 2008), victim/ials.py;
        # seed None = the item table's seed is drawn from torch's global RNG at .I()
        "ials": {"factor_num": 64, "alpha": 40.0, "reg_lambda": 10.0, "init_std": 0.01, "seed": None},
        # build-specific (no reference counterpart): sparse linear item-item weights by coordinate descent (Ning and Karypis 2011),
        # victim/slim.py; l2_reg is the constant added to the Gram matrix's diagonal
        "slim": {"l1_reg": 1.0, "l2_reg": 5.0, "sweeps": 50},
        # build-specific (no reference counterpart): adversarially trained BPR-MF (He, He, Du and Chua 2018), victim/apr.py;
        # adv_reg = 0 is plain BPR-MF; the adversarial term is switched on after adv_start_epoch of the victim's own epochs
        "apr": {"factor_num": 64, "reg_lambda": 1e-4, "eps": 0.5, "adv_reg": 1.0, "adv_start_epoch": 200, "init_std": 0.01,
                "optim": "adam", "lr": 1e-3},
        # build-specific (no reference counterpart): the multinomial variational autoencoder (Liang et al. 2018), victim/multvae.py;
        # seed None = the initialisation's and the device RNG's seed is drawn from torch's global RNG at .I()
        "multvae": {"hidden_dim": 600, "latent_dim": 200, "dropout": 0.5, "anneal_cap": 0.2, "total_anneal_steps": 200000,
                    "batch_size": 500, "optim": "adam", "lr": 1e-3, "seed": None},
        # build-specific (no reference counterpart): the random-walk item-item recommender (P3alpha, Cooper et al. 2014; RP3beta,
        # Christoffel et al. 2015), victim/rp3beta.py; beta = 0 is P3alpha; band None = automatic
        "rp3beta": {"alpha": 1.0, "beta": 0.6, "k": 100, "band": None},
        # build-specific (no reference counterpart): user-neighbourhood CF (Resnick et al. 1994; Herlocker et al. 1999),
        # victim/userknn.py; normalize True = the weighted average (for ratings), band None = automatic
        "userknn": {"k": 50, "normalize": False, "band": None},
    },
    "attacker": {
        "random": {"attack_num": 50, "filler_num": 36},
        # recad/default.py:136-158; seed as for aush.  The reference's BandwagonAttack reads the segment entry by mistake
        # (heuristic.py:264-266); here bandwagon reads its own, so an empty selected_ids means the 11 most rated items
        "average": {"attack_num": 50, "filler_num": 36, "seed": None},
        "segment": {"attack_num": 50, "filler_num": 36,
                    "selected_ids": [1153, 2201, 1572, 836, 523, 849, 1171, 344, 857, 1213, 1535], "seed": None},
        "bandwagon": {"attack_num": 50, "filler_num": 36, "selected_ids": [], "seed": None},
        # recad/default.py:159-168; seed is this build's: the key of the device RNG (None = drawn from np.random at .I())
        "aush": {"attack_num": 50, "filler_num": 36, "lr_g": 0.01, "lr_d": 0.001, "optim_g": "adam", "optim_d": "adam",
                 "selected_ids": [62], "ZR_ratio": 0.2, "seed": None},
        # recad/default.py:169-186; history_bytes is this build's: the cap of the unrolled epochs' stored states (theta, m, v per
        # step); above it the reverse pass keeps a checkpoint every ceil(sqrt(K)) steps and re-runs each segment forward
        "aia": {"attack_num": 50, "filler_num": 36, "lr_g": 0.01, "lr_d": 0.001, "optim_g": "adam", "optim_d": "adam",
                "surrogate_model": "WMF", "epoch_s": 50, "unroll_steps_s": 1, "hidden_dim_s": 16, "lr_s": 1e-2,
                "weight_decay_s": 1e-5, "batch_size_s": 16, "weight_pos_s": 1.0, "weight_neg_s": 0.0, "selected_ids": [62],
                "history_bytes": 1 << 30},
        # recad/default.py:187-209 (pretrain_epoch_d is there and never read); history_bytes as for aia
        "aushplus": {"attack_num": 50, "pretrain_epoch_g": 1, "pretrain_epoch_d": 5, "epoch_gan_d": 5, "epoch_gan_g": 1,
                     "epoch_surrogate": 50, "filler_num": 36, "lr_g": 0.01, "lr_d": 0.001, "optim_g": "adam", "optim_d": "adam",
                     "surrogate_model": "WMF", "epoch_s": 50, "unroll_steps_s": 1, "hidden_dim_s": 16, "lr_s": 1e-2,
                     "weight_decay_s": 1e-5, "batch_size_s": 16, "weight_pos_s": 1.0, "weight_neg_s": 0.0, "selected_ids": [62],
                     "history_bytes": 1 << 30},
        # recad/default.py:210-221; hops and seed are this build's: "elementwise" is uba.py:99 as written, "matrix" the three-hop
        # product its names promise (attack/uba.py); seed as for aush, also the key of the budget redraws
        "uba": {"attack_num": 50, "filler_num": 36, "lr_g": 0.01, "lr_d": 0.001, "optim_g": "adam", "optim_d": "adam",
                "selected_ids": [62], "ZR_ratio": 0.2,
                "target_user_ids": [741, 225, 289, 338, 308, 244, 605, 86, 46, 570, 208, 972, 21, 284, 578, 616, 103, 981, 18, 383, 432,
                                    454, 835, 14, 537, 500, 486, 318, 754, 385, 218, 545, 154, 226, 301, 469, 92, 617, 728, 926, 651, 725,
                                    418, 435, 243, 595, 97, 130, 836, 91],
                "budget": 6, "hops": "elementwise", "seed": None},
        # build-specific (no reference counterpart): projected gradient ascent through one sweep of an iALS surrogate (Li, Wang,
        # Singh and Vorobeychik 2016), attack/pga.py.  These values are choices, not tuned ones: nobody has measured which
        # settings attack best.  seed_s None = the surrogate's item table is seeded from torch's global RNG at .I()
        "pga": {"attack_num": 50, "filler_num": 36, "fake_rating": 5.0, "lr": 0.25, "factor_num_s": 16, "alpha_s": 40.0,
                "reg_lambda_s": 10.0, "init_sweeps_s": 10, "sweeps_s": 2, "seed_s": None},
    },
    # recad/default.py:223-228; block / tol / max_iter / seed are this build's solver knobs (block None = 8, or 16 when kVals > 5)
    "defender": {"PCASelectUsers": {"kVals": 3, "attack_num": 50, "block": None, "tol": 1e-5, "max_iter": 300, "seed": SEED},
                 # build-specific (no reference counterpart): DegSim neighbour detection, defense/knn_select_users.py
                 "KnnSelectUsers": {"k": 25, "attack_num": 50, "select": "low", "band": None, "schedule": "work"},
                 # build-specific (no reference counterpart): CatchSync synchronicity detection, defense/catchsync_select_users.py;
                 # form None = automatic by row length
                 "CatchSyncSelectUsers": {"score": "sync", "grid_bits": 1, "min_items": 20, "attack_num": 50, "schedule": "work",
                                          "form": None},
                 # build-specific (no reference counterpart): FRAUDAR dense-block peeling, defense/fraudar_select_users.py
                 "FraudarSelectUsers": {"weight": "log", "log_offset": 5.0, "select": "block", "n_blocks": 1, "attack_num": 50}},
}
for _scope in MODEL.values():
    for _cfg in _scope.values():
        _cfg["logging_level"] = logging.INFO
        _cfg["device"] = DEVICE

DATASET_IMPLICIT = {
    "path_train": None, "path_valid": None, "path_test": None,
    "test_batch_size": 400, "A_split": False, "A_n_fold": 100,
    "pairwise_batch_size": 1024, "pointwise_batch_size": 1024, "sample": "pairwise", "negative_ratio": 4,
    "need_graph": True, "rating_filter": 4,
    "logging_level": logging.INFO, "train_dict": None, "valid_dict": None, "test_dict": None,
    "device": DEVICE, "if_cache": False, "cache_dir": os.path.join(".", "generated"),
    # build-specific (no reference counterpart):
    "graph_source": "reference",  # "reference" = adjacency/positives from the LAST split read (test); "train"
    "sampler": "auto",            # "numpy" (vectorised host) | "device" (HIP) | "auto" = device when on a GPU
}

# recad/default.py:67-89 (the "explicit" scope) and the keys _decorate_config adds (:92-99)
DATASET_EXPLICIT = {
    "path_train": None, "path_test": None, "path_valid": None,
    "batch_size": 256, "header": None, "sep": ",", "threshold": 4, "sample": "row",
    "logging_level": logging.INFO, "train_dict": None, "valid_dict": None, "test_dict": None, "remap_enable": False,
    "device": DEVICE, "if_cache": False, "cache_dir": os.path.join(".", "generated"),
    # build-specific (no reference counterpart):
    "train_csr": None, "valid_csr": None, "test_csr": None,   # (ptr, idx, val) rating CSRs
    "user_map": None,             # set by partial_sample: the remap it applied
    "dense_limit": 1 << 28,       # train_mat (dense U x I float32) is refused above this many entries (1 GiB)
}

WORKFLOW = {
    "no defense": {
        "rec_epoch": 400, "attack_epoch": 100, "target_id_list": [0], "filter_num": 4, "topks": [10, 20, 50, 100],
        "logging_level": logging.INFO, "device": DEVICE, "cache_dir": os.path.join(".", "workflows_results"),
        "quality_split": None,        # build-specific: None | "valid" | "test" = also report held-out Recall / NDCG / ... @k
    },
    "defense": {
        "rec_epoch": 400, "attack_epoch": 100, "target_id_list": [0], "filter_num": 4, "topks": [10, 20, 50, 100],
        "defense_epoch": 1,
        "logging_level": logging.INFO, "device": DEVICE, "cache_dir": os.path.join(".", "workflows_results"),
        "quality_split": None,        # build-specific: None | "valid" | "test" = also report held-out Recall / NDCG / ... @k
    },
    # build-specific: one clean victim, one poisoned retrain per case {"attacker", "target_id_list"} (workflow.Sweep)
    "sweep": {
        "rec_epoch": 400, "attack_epoch": 100, "filter_num": 4, "topks": [10, 20, 50, 100],
        "logging_level": logging.INFO, "device": DEVICE, "cache_dir": os.path.join(".", "workflows_results"),
        "quality_split": None,
        "group": 8,                   # poisoned victims retrained per train_group call (victims that have one); 1 = one after another
    },
}


def set_device_id(cuda_id):
    """recad/default.py:285-290."""
    device = torch.device(f"cuda:{cuda_id}" if torch.cuda.is_available() else "cpu")
    for scope in MODEL.values():
        for cfg in scope.values():
            cfg["device"] = device
    DATASET_IMPLICIT["device"] = device
    DATASET_EXPLICIT["device"] = device
    for cfg in WORKFLOW.values():
        cfg["device"] = device
    return device
