"""Command line of the trainer: the flags of learning/OieInduction.py:461-500 (same names,
defaults and meaning), plus the README's aliases (README.md:44: --pickled_dataset,
--model_name, --batch_size, --relations_number, --negative_samples_number,
--l2_regularization, --embed_size, --learning_rate, --optimization).

    python -m rae DATASET --model-name NAME --decoder sp [--epochs 100 ...]

DATASET is a preprocessed file written by ``python -m rae.preprocess`` (.json / .json.gz: the
reference's OiePreprocessor output, stored without pickles), an array dataset written by
rae.data.save_npz, or ``synthetic:N[:d[:K]]`` for the SURVEY 8(d) generator.  Multi-GPU: launch with torch.distributed.run, one process per GPU.
"""
from __future__ import annotations

import argparse
import sys

import numpy as np


def _str_bool(v):
    """learning/OieInduction.py fix_parsing: 'True'/'False' strings from store_true defaults."""
    if isinstance(v, bool):
        return v
    return str(v).lower() in ("true", "1", "yes")


def get_command_args(argv=None, program_name="rae"):
    p = argparse.ArgumentParser(prog=program_name,
                                description="Trains a basic Open Information Extraction Model",
                                formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("dataset", nargs="?", default=None,
                   help="preprocessed .json[.gz] (rae.preprocess), dataset .npz "
                        "(rae.data.save_npz) or synthetic:N[:d[:K]]")
    p.add_argument("--pickled_dataset", dest="dataset_alias", default=None, help=argparse.SUPPRESS)
    p.add_argument("--epochs", type=int, default=100, help="the number of training epochs")
    p.add_argument("--learning-rate", "--learning_rate", dest="learning_rate", type=float,
                   default=0.1, help="the initial learning rate")
    p.add_argument("--batch-size", "--batch_size", dest="batch_size", type=int, default=50,
                   help="the size of the minibatches (per GPU)")
    p.add_argument("--embed-size", "--embed_size", dest="embed_size", type=int, default=30,
                   help="the embedding space dimensionality")
    p.add_argument("--relations", "--relations_number", dest="relations", type=int, default=3,
                   help="the number of semantic relation to induce")
    p.add_argument("--neg-samples", "--negative_samples_number", dest="neg_samples", type=int,
                   default=5, help="the number of negative samples to take per entity")
    p.add_argument("--l1", metavar="lambda_1", type=float, default=0.0,
                   help="the value of the L1-norm regularization coefficient")
    p.add_argument("--l2", "--l2_regularization", metavar="lambda_2", dest="l2", type=float,
                   default=0.0, help="the value of the L2-norm regulatization coefficient")
    p.add_argument("--optimizer", choices=["adagrad", "sgd"], type=str, default="adagrad",
                   help="the optimization algorithm")
    p.add_argument("--optimization", type=int, default=None, help=argparse.SUPPRESS)
    p.add_argument("--model-name", "--model_name", dest="model_name", type=str, default=None,
                   help="a name to be given to the trained model instance")
    p.add_argument("--model", dest="legacy_model", default=None, help=argparse.SUPPRESS)
    p.add_argument("--decoder", choices=["rescal", "sp", "rescal+sp"], type=str,
                   help="the type of factorization model to be used as the decoder")
    p.add_argument("--ext-emb", dest="ext_emb", action="store_true", default="False",
                   help="use external embeddings (not supported: SURVEY 8a11 marks it out)")
    p.add_argument("--ext-reg", dest="ext_reg", action="store_true", default="True",
                   help="regularize the factorization (decoder) model parameters as well")
    p.add_argument("--freq-eval", dest="freq_eval", action="store_true", default="False",
                   help="use frequent evaluation")
    p.add_argument("--alpha", type=float, default=1.0,
                   help="the alpha coefficient for scaling the entropy term")
    p.add_argument("--seed", type=int, default=2, help="a seed number")
    p.add_argument("--graph-chunk", type=int, default=64,
                   help="training steps captured per HIP graph (1 = eager launches)")
    p.add_argument("--eval-cost", dest="eval_cost", action="store_true", default=False,
                   help="after each epoch also report the forward-only objective of the "
                        "evaluated splits (train, or valid and test)")
    p.add_argument("--eval-seed", dest="eval_seed", type=int, default=None,
                   help="key of the fixed negatives the objective is scored against")
    p.add_argument("--eval-rank", dest="eval_rank", action="store_true", default=False,
                   help="after each epoch also rank the true arguments of the evaluated splits "
                        "among all entities (MRR, mean rank, hits@k, exact log-likelihood)")
    p.add_argument("--eval-rank-ks", dest="eval_rank_ks", type=_int_list, default=(1, 10, 100),
                   help="comma-separated hits@k thresholds of --eval-rank (at most four)")
    p.add_argument("--eval-rank-rows", dest="eval_rank_rows", type=int, default=None,
                   help="rank only the first N rows of each split (default: the whole split)")
    p.add_argument("--print-preferences", dest="print_preferences", type=int, nargs="?",
                   const=5, default=0, metavar="N",
                   help="after each evaluation print every induced relation's N (default 5, "
                        "1..32) highest-scoring entities per argument slot with their scores "
                        "(sp and rescal+sp)")
    p.add_argument("--print-features", dest="print_features", type=int, nargs="?",
                   const=10, default=0, metavar="N",
                   help="after each evaluation print every induced relation's N (default 10, "
                        "1..32) features with the highest row-centred encoder weight, with "
                        "that weight and the feature's count in the training split")
    p.add_argument("--print-features-min-count", dest="print_features_min_count", type=int,
                   default=5, metavar="C",
                   help="--print-features ranks only features in at least C training rows "
                        "(a rare feature carries a large, meaningless weight)")
    p.add_argument("--print-features-raw", dest="print_features_raw", action="store_true",
                   help="--print-features ranks by W[f, k] itself, not the row-centred weight")
    p.add_argument("--print-exemplars", dest="print_exemplars", type=int, nargs="?",
                   const=5, default=0, metavar="N",
                   help="after each evaluation print every induced relation's N (default 5, "
                        "1..32) most confident rows of the evaluated splits as "
                        "row:e1 | trigger | e2:score.  Always over the encoder's own labels, "
                        "whatever --label-with is: the margin is the encoder's statement about "
                        "its own argmax")
    p.add_argument("--print-exemplars-order", dest="print_exemplars_order", default="most",
                   choices=("most", "least", "both"),
                   help="--print-exemplars lists the most confident rows of a relation, the "
                        "least confident (its boundary), or both")
    p.add_argument("--print-exemplars-by", dest="print_exemplars_by", default="margin",
                   choices=("margin", "pmax"),
                   help="--print-exemplars ranks by the encoder's logit margin (best minus "
                        "second-best logit: it still separates rows whose posterior is 1.0) or "
                        "by its posterior of the label")
    p.add_argument("--predict-arguments", dest="predict_arguments", type=int, default=0,
                   metavar="ROWS",
                   help="after the last epoch print the model's top predictions for both "
                        "arguments of the first ROWS rows of the evaluated splits, beside the "
                        "true argument")
    p.add_argument("--predict-top", dest="predict_top", type=int, default=10, metavar="N",
                   help="predictions printed per row and side by --predict-arguments (1..32)")
    p.add_argument("--predict-relations", dest="predict_relations", type=int, default=0,
                   metavar="ROWS",
                   help="after the last epoch print, for the first ROWS rows of the evaluated "
                        "splits, the two entities, the encoder's label and probability, the "
                        "--predict-top relations the decoder scores highest for the pair, and "
                        "the joint label")
    p.add_argument("--label-with", dest="label_with", choices=["encoder", "decoder", "joint"],
                   default="encoder",
                   help="which labels the cluster evaluation and the printed clusters are built "
                        "from: the encoder's argmax, the decoder's best relation for the two "
                        "arguments, or the argmax of their joint score")
    p.add_argument("--cluster-eval", dest="cluster_eval", choices=["host", "device"],
                   default="host",
                   help="where the induced clusters are scored: the host evaluator, or the "
                        "contingency table and B^3 on the GPU")
    p.add_argument("--print-clusters", dest="print_clusters", choices=["off", "host", "device"],
                   default="off",
                   help="after each evaluation print every induced relation's most frequent "
                        "triggers with their frequencies: from downloaded labels on the host, "
                        "or by the key table and top-k kernels on the GPU")
    p.add_argument("--print-top", dest="print_top", type=int, default=5,
                   help="triggers printed per relation (1..32)")
    p.add_argument("--print-clusters-by", dest="print_by", choices=["trigger", "gold"],
                   default="trigger",
                   help="what is counted per relation: the examples' triggers (needs a dataset "
                        "written by rae.preprocess) or their first gold labels")
    if argv is not None and len(argv) == 0:
        p.print_help()
        raise SystemExit(1)
    a = p.parse_args(argv)
    if a.dataset is None:
        a.dataset = a.dataset_alias
    if a.dataset is None:
        p.error("a dataset is required")
    if a.model_name is None:
        p.error("--model-name is required")
    if a.optimization is not None:        # README.md:44 --optimization 1 (AdaGrad) / 0 (SGD)
        a.optimizer = "adagrad" if a.optimization else "sgd"
    if a.decoder is None:
        p.error("--decoder is required (rescal, sp or rescal+sp)")
    a.ext_emb = _str_bool(a.ext_emb)
    a.ext_reg = _str_bool(a.ext_reg)
    a.freq_eval = _str_bool(a.freq_eval)
    if a.ext_emb:
        p.error("--ext-emb (gensim external embeddings) is out of scope")
    return a


def _int_list(text):
    try:
        ks = tuple(int(x) for x in text.split(",") if x.strip())
    except ValueError:
        raise argparse.ArgumentTypeError(f"not a comma-separated list of integers: {text!r}")
    if not 1 <= len(ks) <= 4 or any(k < 1 for k in ks):
        raise argparse.ArgumentTypeError("one to four thresholds, each >= 1")
    return ks


def load_dataset(spec: str, seed: int = 1234):
    from .data import load_npz, synthetic_dataset
    if spec.startswith("synthetic:"):
        parts = [int(x) for x in spec.split(":")[1:]]
        N = parts[0]
        d = parts[1] if len(parts) > 1 else 2 ** 17
        K = parts[2] if len(parts) > 2 else 10
        return synthetic_dataset(N, d, K, seed=seed)
    if spec.endswith((".json", ".json.gz")):
        from .preprocess import load_data
        return load_data(spec)
    return load_npz(spec)


def main(argv=None):
    args = get_command_args(sys.argv[1:] if argv is None else argv)
    import torch

    from . import dist as rdist
    from .inducer import ReconstructInducer
    ws, rk, lrank = rdist.init()
    dev = torch.device("cuda", lrank)
    torch.cuda.set_device(dev)
    print("Relation Learner", file=sys.stderr)
    rand = np.random.RandomState(seed=args.seed)
    data, gold = load_dataset(args.dataset)
    exchange = rdist.make_exchange(ws, rk)
    ind = ReconstructInducer(data, gold, rand, args.epochs, args.learning_rate, args.batch_size,
                             args.embed_size, args.relations, args.neg_samples, args.l1, args.l2,
                             args.optimizer, args.model_name, args.decoder, args.ext_emb,
                             args.ext_reg, args.freq_eval, args.alpha, device=dev, world_size=ws,
                             rank=rk, exchange=exchange, graph_chunk=args.graph_chunk,
                             eval_cost=args.eval_cost, eval_seed=args.eval_seed,
                             cluster_eval=args.cluster_eval,
                             print_clusters=args.print_clusters, print_top=args.print_top,
                             print_by=args.print_by, eval_rank=args.eval_rank,
                             eval_rank_ks=args.eval_rank_ks, eval_rank_rows=args.eval_rank_rows,
                             print_preferences=args.print_preferences,
                             predict_arguments=args.predict_arguments,
                             predict_top=args.predict_top,
                             label_with=args.label_with,
                             predict_relations=args.predict_relations,
                             print_features=args.print_features,
                             print_features_min_count=args.print_features_min_count,
                             print_features_raw=args.print_features_raw,
                             print_exemplars=args.print_exemplars,
                             print_exemplars_order=args.print_exemplars_order,
                             print_exemplars_by=args.print_exemplars_by)
    if exchange is not None:
        ind.compile_function()
        rdist.warm_up(exchange, ind.engine.exchange_buf)
    ind.train()
    return ind


if __name__ == "__main__":
    main()
