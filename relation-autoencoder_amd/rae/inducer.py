"""ReconstructInducer: the trainer that drives the training path
(learning/OieInduction.py:26-319), same constructor, same ``func`` dictionary, same epoch
loop and RNG consumption -- with the step running on MI355X.
"""
from __future__ import annotations

import sys
import time
from collections import Counter

import numpy as np
import torch

from .data import SPLIT_LABELS
from .engine import DeviceSplit, TrainEngine
from .evaluation import (GoldIndex, KeyIndex, construct_split_evaluator,
                         format_argument_predictions, format_cluster_exemplars,
                         format_cluster_profiles,
                         format_relation_features, format_relation_predictions,
                         format_relation_preferences, key_table, row_keys, topk_from_table)
from .model import OieModelFunctions, _as_bool, make_optimizer
from .negatives import NegativeExampleGenerator


class _TrainFunction:
    """``func['train'](batch_index, neg1, neg2) -> cost`` (OieInduction.py:146-149)."""

    def __init__(self, engine):
        self.engine = engine

    def __call__(self, batch_index, neg1, neg2):
        return self.engine.train_call(batch_index, neg1, neg2)


class _LabelFunction:
    """``func['label_<split>'](batch_index) -> (labels, probs)`` (OieInduction.py:151-155)."""

    def __init__(self, engine, split, batch_size):
        self.engine = engine
        self.split = split
        self.l = batch_size

    def __call__(self, batch_index):
        b = int(batch_index)
        lab, pr = self.engine.label(self.split, b * self.l, self.l)
        return lab.cpu().numpy(), pr.cpu().numpy()

    def all_labels(self, nb_batches):
        """Labels of the first nb_batches*l rows in one launch (tail dropped as the
        reference's per-batch loop does, OieInduction.py:337)."""
        lab, _ = self.engine.label(self.split, 0, nb_batches * self.l, probs=False)
        return lab.cpu().numpy()


class _CostFunction:
    """``func['cost_<split>'](batch_index, neg1, neg2) -> cost``: func['train']'s signature and
    batch slicing (rows [b*l, (b+1)*l), (s, l) negatives) without the update -- the data term
    of the cost (no L1 / L2), by rae_eval_cost (TrainEngine.evaluate)."""

    def __init__(self, engine, split, batch_size):
        self.engine = engine
        self.split = split
        self.l = batch_size

    def __call__(self, batch_index, neg1, neg2):
        b = int(batch_index)
        if not 0 <= b < self.split.N // self.l:
            raise IndexError(f"batch index {b} out of range [0, {self.split.N // self.l})")
        return self.engine.evaluate(self.split, b * self.l, self.l, neg1, neg2,
                                    neg_per_call=True).cost


class ReconstructInducer:
    def __init__(self, data, gold_standard, rng, nb_epochs, learning_rate, batch_size,
                 embed_size, nb_relations, nb_neg_samples, lambda1, lambda2, optimization,
                 model_name, decoder_model, external_embeddings, extended_regularizer,
                 frequent_eval, alpha, *, device=None, world_size=1, rank=0, exchange=None,
                 graph_chunk=64, neg_sampler="device", neg_seed=0, mfma_bf16=False,
                 kernel_forms=None, dp_update="replicated", index_window=0,
                 index_overlap=True, p2p_cross_device=False, p2p_timeout=5.0,
                 eval_cost=False, eval_seed=None, cluster_eval="host", print_clusters="off",
                 print_top=5, print_by="trigger", eval_rank=False, eval_rank_ks=(1, 10, 100),
                 eval_rank_rows=None, print_preferences=0, predict_arguments=0, predict_top=10,
                 label_with="encoder", predict_relations=0, print_features=0,
                 print_features_min_count=5, print_features_raw=False, print_exemplars=0,
                 print_exemplars_order="most", print_exemplars_by="margin"):
        if label_with not in ("encoder", "decoder", "joint"):
            raise ValueError("label_with must be 'encoder', 'decoder' or 'joint'")
        if int(predict_relations) < 0:
            raise ValueError("predict_relations must be >= 0")
        if not 0 <= int(print_features) <= 32:
            raise ValueError("print_features must be in [0, 32] (0: off)")
        if int(print_features_min_count) < 0:
            raise ValueError("print_features_min_count must be >= 0")
        if not 0 <= int(print_exemplars) <= 32:
            raise ValueError("print_exemplars must be in [0, 32] (0: off)")
        if print_exemplars_order not in ("most", "least", "both"):
            raise ValueError("print_exemplars_order must be 'most', 'least' or 'both'")
        if print_exemplars_by not in ("margin", "pmax"):
            raise ValueError("print_exemplars_by must be 'margin' or 'pmax'")
        if not 0 <= int(print_preferences) <= 32:
            raise ValueError("print_preferences must be in [0, 32] (0: off)")
        if int(predict_arguments) < 0 or not 1 <= int(predict_top) <= 32:
            raise ValueError("predict_arguments must be >= 0 and predict_top in [1, 32]")
        if int(print_preferences) and decoder_model == "rescal":
            raise ValueError("print_preferences needs the selectional-preference matrices "
                             "('sp' or 'rescal+sp')")
        if cluster_eval not in ("host", "device"):
            raise ValueError("cluster_eval must be 'host' or 'device'")
        if print_clusters not in ("off", "host", "device"):
            raise ValueError("print_clusters must be 'off', 'host' or 'device'")
        if print_by not in ("trigger", "gold"):
            raise ValueError("print_by must be 'trigger' or 'gold'")
        if print_clusters != "off":
            if not 1 <= int(print_top) <= 32:
                raise ValueError("print_top must be in [1, 32]")
            if print_by == "trigger" and getattr(data, "featureLex", None) is None:
                raise ValueError("print_clusters by trigger needs the dataset's feature lexicon "
                                 "(a file written by rae.preprocess); this dataset has none -- "
                                 "use print_by='gold'")
        self.data = data
        self.goldStandard = gold_standard
        self.rng = rng
        self.nb_epochs = nb_epochs
        self.learningRate = learning_rate
        self.batch_size = batch_size
        self.embedSize = embed_size
        self.relationNum = nb_relations
        self.neg_sample_num = nb_neg_samples
        self.lambdaL1 = lambda1
        self.lambdaL2 = lambda2
        self.optimization = optimization
        self.modelName = model_name
        self.decoder_type = decoder_model
        self.extEmb = external_embeddings
        self.extendedReg = extended_regularizer
        self.frequentEval = _as_bool(frequent_eval)
        self.alpha = alpha
        self.device = device if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.world_size = int(world_size)
        self.rank = int(rank)
        self.exchange = exchange
        self.graph_chunk = graph_chunk
        if neg_sampler not in ("host", "device", "philox"):
            raise ValueError("neg_sampler must be 'host', 'device' or 'philox'")
        self.neg_sampler = neg_sampler     # host / device: the reference's RNG stream
        self.neg_seed = int(neg_seed)
        self.mfma_bf16 = bool(mfma_bf16)   # RESCAL / hybrid: bf16 MFMA operands (config 5)
        self.kernel_forms = dict(kernel_forms or {})   # engine.TrainEngine kernel_forms
        self.index_window = int(index_window)          # engine.TrainEngine row-index ring
        self.index_overlap = bool(index_overlap)       # next window's index beside the steps
        self.dp_update = dp_update         # "replicated" | "partitioned" (rae/dist.py)
        # peer-to-peer exchange (kernel_forms dp_xchg="p2p"): ranks on different GPUs only
        # when asked for (engine.TrainEngine._p2p_setup); a wait's bound in seconds
        self.p2p_cross_device = bool(p2p_cross_device)
        self.p2p_timeout = float(p2p_timeout)
        # eval_cost: learn() also reports the forward-only objective of the splits it evaluates
        # after each epoch, against negatives fixed by eval_seed (TrainEngine.eval_negatives;
        # every rank scores the whole split)
        self.eval_cost = bool(eval_cost)
        self.eval_seed = eval_seed
        self.eval_costs = {s: [] for s in SPLIT_LABELS}
        # eval_rank: learn() also ranks the true arguments of the splits it evaluates among all
        # entities after each epoch (TrainEngine.rank: MRR, mean rank, hits@k, mean exact
        # log-likelihood); eval_rank_rows: the first N rows only (default: the whole split)
        self.eval_rank = bool(eval_rank)
        self.eval_rank_ks = tuple(int(k) for k in eval_rank_ks)
        if len(self.eval_rank_ks) > 4 or any(k < 1 for k in self.eval_rank_ks):
            raise ValueError("eval_rank_ks: at most four thresholds, each >= 1")
        self.eval_rank_rows = None if eval_rank_rows is None else int(eval_rank_rows)
        self.rank_metrics = {s: [] for s in SPLIT_LABELS}
        # print_preferences: after each epoch's evaluation learn() prints, per induced relation
        # and argument slot, the N highest-scoring entities (TrainEngine.relation_preferences);
        # predict_arguments: after the last epoch, the predict_top best entities for both
        # arguments of the first ROWS rows of the evaluated splits (TrainEngine.predict_arguments)
        self.print_preferences = int(print_preferences)
        self.predict_arguments = int(predict_arguments)
        self.predict_top = int(predict_top)
        # label_with: which labels _labels, get_clusters_sets, the host and device cluster
        # evaluation and the cluster profiles use -- "encoder": argmax of the encoder's logits
        # (rae_label, the reference's); "decoder": the relation the two arguments themselves
        # score highest (argmax psi); "joint": argmax of logsoftmax + l (rae_eval_relations).
        # predict_relations: after the last epoch, per row of the first ROWS rows of the
        # evaluated splits, the encoder's label, the predict_top relations by psi and the joint
        # label (TrainEngine.eval_relations)
        self.label_with = label_with
        self.predict_relations = int(predict_relations)
        # print_features: after each epoch's evaluation learn() prints, per induced relation, the
        # N features the encoder weighs highest for it among those in at least
        # print_features_min_count training rows, with their row-centred weight
        # (print_features_raw: W[f, k] itself) and that count (TrainEngine.relation_features)
        self.print_features = int(print_features)
        self.print_features_min_count = int(print_features_min_count)
        self.print_features_raw = bool(print_features_raw)
        # print_exemplars: after each epoch's evaluation learn() prints, per induced relation of
        # the evaluated splits, its N most confident rows (print_exemplars_order "least": its N
        # boundary rows; "both": the two lists) by the encoder's logit margin (print_exemplars_by
        # "pmax": its posterior), as row:e1 | trigger | e2:score (TrainEngine.cluster_exemplars).
        # Always over the ENCODER's own labels, whatever label_with is: the margin is the
        # encoder's statement about its own argmax
        self.print_exemplars = int(print_exemplars)
        self.print_exemplars_order = print_exemplars_order
        self.print_exemplars_by = print_exemplars_by
        # cluster_eval: where learn() scores the induced clusters -- "host": the label download
        # and the Python sets of the reference (get_clusters_sets + SingleLabelClusterEvaluation);
        # "device": the contingency table and B^3 on the GPU (TrainEngine.cluster_metrics), same
        # rows, same printed lines; self.cluster[split] is then not built
        self.cluster_eval = cluster_eval
        self._gold_index = {}
        # print_clusters: after each f1 line learn() prints, per induced relation, the print_top
        # most frequent triggers (print_by="gold": first gold labels) of its members with their
        # frequencies (Visualizator.print_clusters, evaluation/Visuals.py:8-45) -- "host": from
        # the downloaded labels with the numpy oracles of rae/evaluation.py; "device": the key
        # table and top-k on the GPU (TrainEngine.cluster_profiles); the same lines either way
        self.print_clusters = print_clusters
        self.print_top = int(print_top)
        self.print_by = print_by
        self._key_index = {}
        self._host_keys = {}
        self.negativeSampler = NegativeExampleGenerator(rng, data.negSamplingCum)   # :85
        self.modelID = (f"{decoder_model}_{model_name}_maxepoch{nb_epochs}_lr{learning_rate}"
                        f"_embedsize{embed_size}_l1{lambda1}_l2{lambda2}_opt{optimization}"
                        f"_rel_num{nb_relations}_batch{batch_size}_negs{nb_neg_samples}")
        self.modelFunc = OieModelFunctions(rng, embed_size, nb_relations, nb_neg_samples,
                                           batch_size, decoder_model, data, extended_regularizer,
                                           alpha, external_embeddings=external_embeddings,
                                           device=self.device)          # :90
        self.func = dict(zip([SPLIT_LABELS[0]] + ["label_" + s for s in SPLIT_LABELS],
                             [None] * (1 + len(SPLIT_LABELS))))         # :91
        self.cur_epoch = 0
        self.evaluator = {s: None for s in SPLIT_LABELS}
        for split in self.data.generate_split_keys():
            self.evaluator[split] = construct_split_evaluator(
                (gold_standard or {}).get(split, {}), split)
        self.batch_reps = {s: None for s in SPLIT_LABELS}
        for split in self.data.generate_split_keys():
            # Py2 integer division: tail dropped (:98); data-parallel global batch
            self.batch_reps[split] = self.data.split[split].args1.shape[0] // (
                self.batch_size * (self.world_size if split == "train" else 1))
        self.cluster = {s: None for s in SPLIT_LABELS}
        self.train_errors = []
        self.epoch_costs = []
        self.engine = None
        self.optimizer = None
        self._resume = False        # set by load_checkpoint: keep optimizer state + epoch cursor

    def initialize(self):
        """OieInduction.py:103-108: re-draw all parameters from the shared RNG.  Like the
        reference, the next train()/learn() then starts from epoch 0 with a fresh optimizer
        (compile_function builds a new zero-accumulator AdaGrad, OieInduction.py:137)."""
        self._drop_engine()
        self.optimizer = None
        self._resume = False
        self.cur_epoch = 0
        self.train_errors = []
        self.epoch_costs = []
        self.eval_costs = {s: [] for s in SPLIT_LABELS}
        self.rank_metrics = {s: [] for s in SPLIT_LABELS}
        self.modelFunc = OieModelFunctions(self.rng, self.embedSize, self.relationNum,
                                           self.neg_sample_num, self.batch_size,
                                           self.decoder_type, self.data, self.extendedReg,
                                           self.alpha, external_embeddings=self.extEmb,
                                           device=self.device)

    def _drop_engine(self):
        if self.engine is not None:
            self.engine.close()
        self.engine = None
        self.func = {k: None for k in self.func}

    # ------------------------------------------------------------------ compile
    def compile_function(self):
        """OieInduction.py:118-155: build the train function and one labelling function
        per split."""
        if self.optimizer is None or not self._resume:
            # a fresh zero-accumulator optimizer per compile, as the reference builds one
            # (:137); only a loaded checkpoint keeps its accumulators
            self.optimizer = make_optimizer(self.optimization, self.modelFunc.params)
        self.engine = TrainEngine(self.modelFunc, self.optimizer, self.data.split["train"],
                                  learning_rate=self.learningRate, lambda1=self.lambdaL1,
                                  lambda2=self.lambdaL2, world_size=self.world_size,
                                  rank=self.rank, exchange=self.exchange,
                                  graph_chunk=self.graph_chunk, device=self.device,
                                  mfma_bf16=self.mfma_bf16, kernel_forms=self.kernel_forms,
                                  dp_update=self.dp_update, index_window=self.index_window,
                                  index_overlap=self.index_overlap,
                                  p2p_cross_device=self.p2p_cross_device,
                                  p2p_timeout=self.p2p_timeout)
        self.func["train"] = _TrainFunction(self.engine)
        self.engine.label_with = self.label_with
        self.engine.eval_sampler = self.negativeSampler      # its CDF only (eval_negatives)
        self._dev_split = {}
        for key in self.data.generate_split_keys():
            ds = self.engine.split if key == "train" else DeviceSplit(self.data.split[key], self.device)
            self._dev_split[key] = ds
            self.func["label_" + key] = _LabelFunction(self.engine, ds, self.batch_size)
            self.func["cost_" + key] = _CostFunction(self.engine, ds, self.batch_size)

    def _check_for_compiled_functions(self):
        return self.func.get("train") is not None

    # ------------------------------------------------------------------ train / learn
    def train(self, debug=False):
        """OieInduction.py:157-170 (wall-clock timers instead of process CPU time)."""
        t0 = time.perf_counter()
        if not self._check_for_compiled_functions():
            self.compile_function()
        compile_duration = time.perf_counter() - t0
        t0 = time.perf_counter()
        self.learn(debug=debug)
        train_duration = time.perf_counter() - t0
        print("Compiling completed in {:.1f}s".format(compile_duration), file=sys.stderr)
        print("Training completed in {:.1f}s".format(train_duration), file=sys.stderr)
        if self.cur_epoch:
            print("Trained for {} epochs. Avg epoch duration: {:.1f}s".format(
                self.cur_epoch, train_duration / float(self.cur_epoch)))

    def draw_epoch_negatives(self):
        """OieInduction.py:183-184: neg1 then neg2, each (s, N), from the shared RNG."""
        N = self.data.split["train"].args1.shape[0]
        neg1 = self.negativeSampler.get_negative_samples(N, self.neg_sample_num)
        neg2 = self.negativeSampler.get_negative_samples(N, self.neg_sample_num)
        return neg1, neg2

    def learn(self, debug=False, verbose=True):
        """OieInduction.py:172-219.  Per epoch: draw negatives on the host RNG (parity mode),
        upload once, run every batch on the device, read the per-batch costs back and sum
        them in batch order (err += cost, :189)."""
        if not self._check_for_compiled_functions():
            self.compile_function()
        nb = self.batch_reps["train"]
        # the reference always starts at epoch 0 (:175); a loaded checkpoint resumes at the
        # epoch it was taken at
        epoch = self.cur_epoch if self._resume else 0
        self._resume = False
        while epoch < self.nb_epochs:
            t0 = time.perf_counter()
            epoch += 1
            self.cur_epoch = epoch
            if self.neg_sampler == "host":
                neg1, neg2 = self.draw_epoch_negatives()
                self.engine.set_epoch_negatives(neg1, neg2)
            else:
                self.engine.sample_epoch_negatives(self.negativeSampler, self.neg_sampler,
                                                   self.neg_seed, epoch - 1)
            if self.frequentEval:
                # per-batch evaluation needs the host between batches (:190-198)
                for b in range(nb):
                    self.engine.run(b, 1, graph=False)
                    if self._mode() == 1:
                        print(b * self.batch_size, b, "#" * 60)
                        print(self.get_clusters_size(), "\n")
                    else:                       # mode 2: valid + test after every batch
                        print(b * self.batch_size, b, "#" * 60)
                        for split in SPLIT_LABELS[1:]:
                            self._score(split, verbose=verbose)
            else:
                self.engine.run(0, nb)
            costs = self.engine.costs[:nb].double().cpu().numpy()
            self.engine.check()
            self.epoch_costs.append(costs)
            err = 0.0
            for c in costs:
                err += float(np.float32(c))
            self.train_errors.append(err)
            if verbose:
                print("\nEPOCH", epoch)
                print("Training error: {:.4f}".format(err))
                print("Epoch duration: {:.1f}s".format(time.perf_counter() - t0))
            if self._mode() == 1:
                self._score("train", verbose=verbose)
            else:
                for split in SPLIT_LABELS[1:]:
                    self._score(split, verbose=verbose)
            if self.eval_cost:
                for split in (SPLIT_LABELS[:1] if self._mode() == 1 else SPLIT_LABELS[1:]):
                    self.evaluate_cost(split, verbose=verbose)
            if self.eval_rank:
                for split in (SPLIT_LABELS[:1] if self._mode() == 1 else SPLIT_LABELS[1:]):
                    self.evaluate_rank(split, verbose=verbose)
            # computed whatever `verbose` is, like evaluate_rank: the engine calls may gather stale
            # replicas (a collective), so every rank makes them; only the printing is optional
            if self.print_preferences:
                lines = self.relation_preference_lines()
                if verbose:
                    print("\n".join(lines))
            if self.print_features:
                lines = self.relation_feature_lines()
                if verbose:
                    print("\n".join(lines))
            if self.print_exemplars:
                for split in (SPLIT_LABELS[:1] if self._mode() == 1 else SPLIT_LABELS[1:]):
                    lines = self.cluster_exemplar_lines(split)
                    if verbose:
                        print("\n".join(lines))
        if self.predict_arguments:
            for split in (SPLIT_LABELS[:1] if self._mode() == 1 else SPLIT_LABELS[1:]):
                lines = self.argument_prediction_lines(split)
                if verbose:
                    print("\n".join(lines))
        if self.predict_relations:
            for split in (SPLIT_LABELS[:1] if self._mode() == 1 else SPLIT_LABELS[1:]):
                lines = self.relation_prediction_lines(split)
                if verbose:
                    print("\n".join(lines))
        return self.train_errors

    def relation_preference_lines(self):
        """print_preferences' lines at the current parameters: one per relation and slot."""
        if not self._check_for_compiled_functions():
            self.compile_function()
        ents, scores = self.engine.relation_preferences(self.print_preferences or 5)
        return format_relation_preferences(ents.cpu().numpy(), scores.cpu().numpy(),
                                           getattr(self.data, "id2Arg", None))

    def relation_feature_lines(self):
        """print_features' lines at the current parameters: one per relation, the features' names
        from the dataset's lexicon when it has one (the feature ids otherwise), the counts the
        train split's."""
        if not self._check_for_compiled_functions():
            self.compile_function()
        eng = self.engine
        feats, scores = eng.relation_features(self.print_features or 10,
                                              centre=not self.print_features_raw,
                                              min_support=self.print_features_min_count,
                                              split=eng.split)
        lex = getattr(self.data, "featureLex", None)
        return format_relation_features(feats.cpu().numpy(), scores.cpu().numpy(),
                                        eng.feature_support(eng.split).cpu().numpy(),
                                        lex.get_str_pruned if lex is not None else None)

    def cluster_exemplar_lines(self, split):
        """print_exemplars' lines for the rows _labels covers (the first nbs * batch_size) at the
        current parameters: per order a header, then one line per relation
        (rae.evaluation.format_cluster_exemplars) -- the relation's size under the encoder's
        labels, then its exemplars as row:e1 | trigger | e2:score, the trigger from the dataset's
        lexicon when it has one."""
        if not self._check_for_compiled_functions():
            self.compile_function()
        eng, ds = self.engine, self._dev_split[split]
        nrows = (self.data.split[split].args1.shape[0] // self.batch_size) * self.batch_size
        lab, margin, pmax = eng.label_stats(ds, 0, nrows)
        score = margin if self.print_exemplars_by == "margin" else pmax
        sizes = torch.bincount(lab, minlength=self.relationNum)[:self.relationNum].cpu().numpy()
        row_keys = key_names = None
        if getattr(self.data, "featureLex", None) is not None:
            ki = self._key_index.get("*")
            if ki is None:
                ki = self._key_index["*"] = KeyIndex.from_lexicon(self.data.featureLex)
            if ki.n_keys > 0:
                row_keys, key_names = eng._keys_dev(ds, ki).cpu().numpy(), ki.names
        sp = self.data.split[split]
        note = "" if self.label_with == "encoder" else \
            " (the encoder's own labels, not label_with={})".format(self.label_with)
        lines = []
        for order in (("most", "least") if self.print_exemplars_order == "both"
                      else (self.print_exemplars_order,)):
            res = eng.cluster_exemplars(ds, self.print_exemplars or 5, by=score,
                                        largest=order == "most", labels=lab, row0=0, nrows=nrows)
            lines.append("{} exemplars, {} confident by {}{}".format(
                split, order, self.print_exemplars_by, note))
            lines += format_cluster_exemplars(
                res.rows, res.scores, sizes, np.asarray(sp.args1), np.asarray(sp.args2),
                getattr(self.data, "id2Arg", None), row_keys, key_names)
        return lines

    def argument_prediction_lines(self, split):
        """predict_arguments' lines for the first predict_arguments rows of `split`: a header,
        then one line per row and side."""
        if not self._check_for_compiled_functions():
            self.compile_function()
        ds = self._dev_split[split]
        nrows = max(0, min(ds.N, self.predict_arguments))
        ents, scores = self.engine.predict_arguments(ds, 0, nrows, top=self.predict_top)
        sp = self.data.split[split]
        true = np.stack([np.asarray(sp.args1[:nrows]), np.asarray(sp.args2[:nrows])], axis=1)
        return ["{} predictions ({} rows)".format(split, nrows)] + format_argument_predictions(
            ents.cpu().numpy(), scores.cpu().numpy(), true, getattr(self.data, "id2Arg", None))

    def relation_prediction_lines(self, split):
        """predict_relations' lines for the first predict_relations rows of `split`: a header,
        then one line per row (rae.evaluation.format_relation_predictions)."""
        if not self._check_for_compiled_functions():
            self.compile_function()
        ds = self._dev_split[split]
        nrows = max(0, min(ds.N, self.predict_relations))
        head = "{} relations ({} rows)".format(split, nrows)
        if nrows == 0:
            return [head]
        lab, pr = self.engine.label(ds, 0, nrows)
        psi, _, _, lj = self.engine.eval_relations(ds, 0, nrows)
        lab, pr = lab.cpu().numpy(), pr.cpu().numpy()
        sp = self.data.split[split]
        return [head] + format_relation_predictions(
            np.asarray(sp.args1[:nrows]), np.asarray(sp.args2[:nrows]), lab,
            pr[np.arange(nrows), lab], psi.cpu().numpy(), lj.cpu().numpy(),
            min(self.predict_top, self.relationNum), getattr(self.data, "id2Arg", None))

    def evaluate_cost(self, split, verbose=True):
        """The forward-only objective of the whole `split` at the current parameters, against
        the split's fixed evaluation negatives (eval_seed); appended to eval_costs[split]."""
        if not self._check_for_compiled_functions():
            self.compile_function()
        res = self.engine.evaluate(self._dev_split[split], seed=self.eval_seed)
        self.eval_costs[split].append(res.cost)
        if verbose:
            print("{} objective: {:.6f} (reconstruction {:.6f}, entropy {:.6f})".format(
                split, res.cost, res.reconstruction, res.entropy))
        return res

    def evaluate_rank(self, split, verbose=True):
        """The true arguments of `split` (its first eval_rank_rows rows) ranked among all
        entities at the current parameters; the RankResult is appended to rank_metrics[split]."""
        if not self._check_for_compiled_functions():
            self.compile_function()
        ds = self._dev_split[split]
        nrows = ds.N if self.eval_rank_rows is None else max(0, min(ds.N, self.eval_rank_rows))
        res = self.engine.rank(ds, 0, nrows, ks=self.eval_rank_ks)
        self.rank_metrics[split].append(res)
        if verbose:
            hits = " ".join("hits@{} {:.4f}".format(k, v[2]) for k, v in res.hits.items())
            print("{} ranking: MRR {:.6f} (arg1 {:.6f}, arg2 {:.6f}) mean rank {:.1f} {} "
                  "log-likelihood {:.6f} ({} rows)".format(
                      split, res.mrr[2], res.mrr[0], res.mrr[1], res.mean_rank[2], hits,
                      res.logp[2], res.nrows))
        return res

    # ------------------------------------------------------------------ clusters / eval
    def _labels(self, split):
        nbs = self.data.split[split].args1.shape[0] // self.batch_size
        if self.label_with != "encoder":
            if not self._check_for_compiled_functions():
                self.compile_function()
            return self.engine.label_relations(self._dev_split[split], 0, nbs * self.batch_size,
                                               self.label_with).cpu().numpy()
        return self.func["label_" + split].all_labels(nbs)

    def get_clusters_sets(self, split):
        """get_clusters_sets (OieInduction.py:321-340): cluster id -> set of example ids."""
        clusters = {i: set() for i in range(self.relationNum)}
        for idx, pred in enumerate(self._labels(split)):
            clusters[int(pred)].add(idx)
        return clusters

    def get_clusters_size(self, split="train"):
        """get_clusters_size (OieInduction.py:248-259)."""
        if self.cluster_eval == "device":
            sizes = self._cluster_result(split).sizes
            return Counter({c: int(n) for c, n in enumerate(sizes) if n})
        return Counter(int(x) for x in self._labels(split))

    def _cluster_result(self, split, profiles=False):
        """cluster_eval="device": TrainEngine.cluster_metrics over the rows _labels covers (the
        first nbs * batch_size), against the split's whole gold standard.  profiles: also the
        cluster profiles, from the same labelling pass -> (ClusterResult, ProfileResult)."""
        if not self._check_for_compiled_functions():
            self.compile_function()
        ds = self._dev_split[split]
        gi = self._gold_index.get(split)
        if gi is None:
            gi = self._gold_index[split] = GoldIndex(
                (self.goldStandard or {}).get(split, {}), ds.N)
        nbs = self.data.split[split].args1.shape[0] // self.batch_size
        if profiles and self._keys_of(split).n_keys > 0:
            return self.engine.cluster_metrics_and_profiles(
                ds, gi, self._keys_of(split), 0, nbs * self.batch_size, self.print_top)
        res = self.engine.cluster_metrics(ds, gi, 0, nbs * self.batch_size)
        return (res, None) if profiles else res

    def _score(self, split, verbose=True):
        """learn()'s evaluation of one split: the cluster sets and the host evaluator, or
        (cluster_eval="device") the device metrics."""
        if self.cluster_eval == "host":
            self.cluster[split] = self.get_clusters_sets(split)
        return self._evaluate(split, verbose=verbose)

    def _evaluate(self, split, verbose=True):
        ev = self.evaluator.get(split)
        if ev is None:
            return None
        profiles = None
        if self.cluster_eval == "device":
            if verbose and self.print_clusters == "device":    # one labelling pass for both
                res, profiles = self._cluster_result(split, profiles=True)
            else:
                res = self._cluster_result(split)
            f1, pre, rec = res.f1, res.precision, res.recall
        else:
            ev.feed_induced_clusters(self.cluster[split])
            f1, pre, rec = ev.compute_metrics()
        if verbose:
            print("{} f1: {:.4f} pre: {:.4f} rec: {:.4f}".format(split, f1, pre, rec))
            if self.print_clusters != "off":
                for line in self.cluster_profile_lines(split, profiles):
                    print(line)
        return f1, pre, rec

    def _keys_of(self, split):
        """The split's KeyIndex: the lexicon's triggers (one index for every split) or the
        split's first gold labels."""
        tag = split if self.print_by == "gold" else "*"
        ki = self._key_index.get(tag)
        if ki is None:
            if self.print_by == "gold":
                ki = KeyIndex.from_gold((self.goldStandard or {}).get(split, {}),
                                        self.data.split[split].args1.shape[0])
            else:
                ki = KeyIndex.from_lexicon(self.data.featureLex)
            self._key_index[tag] = ki
        return ki

    def cluster_profile_lines(self, split, profiles=None):
        """print_clusters' lines for the rows _labels covers (the first nbs * batch_size): one
        per cluster id, `print_top` (name, frequency) tuples each."""
        ki = self._keys_of(split)
        nrows = (self.data.split[split].args1.shape[0] // self.batch_size) * self.batch_size
        if ki.n_keys == 0:                       # nothing to count: every cluster prints empty
            return format_cluster_profiles([[]] * self.relationNum, [[]] * self.relationNum, [])
        if profiles is None and self.print_clusters == "device":
            if not self._check_for_compiled_functions():
                self.compile_function()
            profiles = self.engine.cluster_profiles(self._dev_split[split], ki, 0, nrows,
                                                    self.print_top)
        if profiles is None:
            keys = self._host_keys.get(split)
            if keys is None:
                keys = ki.rows if ki.rows is not None else \
                    row_keys(self.data.split[split].xFeats, ki.key_of_feature)
                self._host_keys[split] = keys
            table = key_table(self._labels(split), keys[:nrows], self.relationNum, ki.n_keys)
            profiles = topk_from_table(table, self.print_top)
        return format_cluster_profiles(profiles[0], profiles[1], ki.names)

    def _mode(self):
        """OieInduction.py:300-312."""
        if len(self.data.split) == 1 and "train" in self.data.split:
            return 1
        if len(self.data.split) == 3 and all(k in self.data.split for k in SPLIT_LABELS):
            return 2
        raise Exception("Either 'train' split or 'train', 'valid' and 'test' splits should be defined")

    def gather(self):
        """Make this rank's replica whole (partitioned data-parallel update: every A / Ab / W
        row and accumulator from its owner).  A collective -- call it on EVERY rank, e.g. before
        a rank-0-only save_checkpoint or labelling pass; a no-op when nothing is stale and for
        the replicated update."""
        if self.engine is not None:
            self.engine.sync_replicas(accumulators=True)

    def state_dict(self):
        """Parameters + AdaGrad accumulators + RNG state + epoch cursor (the reference's
        save() keeps only the parameters and loses the accumulators and the RNG position,
        OieInduction.py:110-116, so a reloaded model cannot continue the same run).
        Partitioned data-parallel update: if rows are stale this gathers them (a collective:
        all ranks must call it) -- call gather() on every rank first to save from one rank."""
        if self.engine is not None and self.engine.stale(accumulators=True):
            self.engine.sync_replicas(accumulators=True)
        sd = {"params": {k: v.detach().cpu() for k, v in self.modelFunc.named_params().items()},
              "rng": self.rng.get_state(), "epoch": self.cur_epoch,
              "train_errors": list(self.train_errors)}
        if self.optimizer is not None and self.optimizer.accumulator is not None:
            sd["acc"] = {k: v.detach().cpu() for k, v in
                         zip(self.modelFunc.param_names, self.optimizer.accumulator)}
        return sd

    def save_checkpoint(self, path):
        """state_dict() as a flat .npz (no pickles)."""
        sd = self.state_dict()
        name, key, pos, has_gauss, gauss = sd["rng"]
        out = {"epoch": np.int64(sd["epoch"]), "train_errors": np.array(sd["train_errors"]),
               "rng_key": key, "rng_pos": np.int64(pos), "rng_has_gauss": np.int64(has_gauss),
               "rng_gauss": np.float64(gauss), "decoder": np.str_(self.decoder_type)}
        for k, v in sd["params"].items():
            out["param/" + k] = v.numpy()
        for k, v in sd.get("acc", {}).items():
            out["acc/" + k] = v.numpy()
        np.savez(path, **out)

    def load_checkpoint(self, path):
        """Restore a save_checkpoint() file into this inducer (same shapes/decoder): the
        parameters and accumulators are copied into the existing device tensors (a built
        engine keeps its pointers), the shared RNG resumes its stream and learn() continues
        at the next epoch."""
        z = np.load(path, allow_pickle=False)
        if str(z["decoder"]) != self.decoder_type:
            raise ValueError(f"checkpoint decoder {z['decoder']} != {self.decoder_type}")
        for k, v in self.modelFunc.named_params().items():
            v.copy_(torch.as_tensor(z["param/" + k]))
        if self.optimizer is None and self.optimization is not None:
            self.optimizer = make_optimizer(self.optimization, self.modelFunc.params)
        if self.optimizer is not None and self.optimizer.accumulator is not None:
            for k, v in zip(self.modelFunc.param_names, self.optimizer.accumulator):
                v.copy_(torch.as_tensor(z["acc/" + k]))
        self.rng.set_state(("MT19937", z["rng_key"], int(z["rng_pos"]), int(z["rng_has_gauss"]),
                            float(z["rng_gauss"])))
        self.cur_epoch = int(z["epoch"])
        self.train_errors = [float(x) for x in z["train_errors"]]
        self._resume = True
