"""Coordinator: dispatch, cross-agent correlation, root causes (+ device PageRank ranking).

Reference: ref:agents/coordinator.py:7-192.  ``run_analysis`` / the comprehensive result
schema / ``_correlate_findings`` (group by component, first-seen order, max severity by
:data:`SEVERITY_ORDER`) / ``_identify_root_causes`` (critical|high with >1 finding) are kept
exactly.  New, additive: ``ranked_root_causes`` — the root-cause ranking
of krca.rca.Config (the same definition bench.py and RcaStep use: alpha 0.5, p ∝ max(s - floor, 0)
with the scale-aware floor of Config.floor -- the expected maximum |z| of that many null series,
at least 4 -- 30 iterations, key "explained": the mass a pod received from its callers times the
part of its anomaly no anomalous dependency explains) over the dependency graph, seeded by the metrics agent's anomaly scores
(bulk path) or by the trace backend's per-service error rates (C1 mock; error rates are not in
|z| units, so that path seeds with floor 0), computed by ``krca_ppr`` on the device.
"""
import numpy as np

from .base import SEVERITY_ORDER
from .events import EventsAgent
from .logs import LogsAgent
from .metrics import MetricsAgent
from .topology import TopologyAgent, csr_from_edges
from .traces import TracesAgent


class Coordinator:
    def __init__(self, k8s_client, engine=None, rank_config=None, correlations=False, corr_channel=0, corr_span=None,
                 corr_max_lag=8, corr_tau=0.5, corr_slack=0, blast_radius=False, blast_bins=16, level_shifts=False,
                 peer_deviations=False, **shift_options):
        from krca.rca import RANKING
        self.k8s_client = k8s_client
        self._engine = engine
        self.rank_config = rank_config or RANKING
        # correlations=True: the comprehensive result gains the additive key "correlations" (lead/lag
        # correlation of metric channel corr_channel along the dependency edges, krca_corr_edges)
        self.correlations = bool(correlations)
        self.corr_params = {'channel': int(corr_channel), 'span': None if corr_span is None else int(corr_span),
                            'max_lag': int(corr_max_lag), 'tau': float(corr_tau), 'slack': int(corr_slack)}
        # blast_radius=True: the additive key "blast_radius" (what each ranked root cause takes down:
        # krca_graph_reach / krca_graph_reach_cover over the dependency graph)
        self.blast_radius = bool(blast_radius)
        self.blast_bins = int(blast_bins)
        self._rank_ctx = None
        # level_shifts=True: the metrics agent also scores level shifts (its "level_shifts" key; shift_*
        # options are passed through to it) and the comprehensive result gains the additive key
        # "level_shift_root_causes": the same ranking seeded with the shift score
        self.level_shifts = bool(level_shifts)
        # peer_deviations=True: the metrics agent also scores pods against their replicas and nodes against
        # nodes (its "peer_deviations" / "service_wide" / "node_deviations" keys; peer_* options and
        # node_threshold are passed through) and the comprehensive result gains the additive keys
        # "peer_root_causes" (the same ranking seeded with the peer score) and "node_deviations" 
        self.peer_deviations = bool(peer_deviations)
        self.metrics_agent = MetricsAgent(k8s_client, engine, window=self.rank_config.window,
                                          z_threshold=self.rank_config.z_threshold, level_shift=self.level_shifts,
                                          peer_deviation=self.peer_deviations, **shift_options)
        self.logs_agent = LogsAgent(k8s_client, engine)
        self.traces_agent = TracesAgent(k8s_client, engine)
        self.topology_agent = TopologyAgent(k8s_client, engine)
        self.events_agent = EventsAgent(k8s_client, engine)
        self.agent_map = {
            'comprehensive': self._run_comprehensive_analysis,
            'metrics': self.metrics_agent.analyze,
            'logs': self.logs_agent.analyze,
            'traces': self.traces_agent.analyze,
            'topology': self.topology_agent.analyze,
            'events': self.events_agent.analyze,
        }

    @property
    def engine(self):
        if self._engine is None:
            from krca import native
            self._engine = native.default_engine()
        return self._engine

    def run_analysis(self, analysis_type, namespace, context=None, **kwargs):  # ref :39-70
        try:
            if analysis_type not in self.agent_map:
                return {'error': f"Unknown analysis type: {analysis_type}"}
            results = self.agent_map[analysis_type](namespace=namespace, context=context, **kwargs)
            results['metadata'] = {'analysis_type': analysis_type, 'namespace': namespace,
                                   'context': context or self.k8s_client.get_current_context(),
                                   'timestamp': self.k8s_client.get_current_time()}
            return results
        except Exception as e:
            return {'error': str(e)}

    def _run_comprehensive_analysis(self, namespace, context=None, **kwargs):  # ref :72-116
        self._reset_agents()
        order = ('metrics', 'logs', 'topology', 'events', 'traces')
        agents = {'metrics': self.metrics_agent, 'logs': self.logs_agent, 'topology': self.topology_agent,
                  'events': self.events_agent, 'traces': self.traces_agent}
        results = {k: agents[k].analyze(namespace, context, **kwargs) for k in order}
        correlated = self._correlate_findings(*(results[k].get('findings', []) for k in order))
        out = {'correlated_findings': correlated, 'agent_results': results,
               'root_causes': self._identify_root_causes(correlated)}
        ranked = self._rank_root_causes(namespace)
        if ranked is not None:
            out['ranked_root_causes'] = ranked
        if self.blast_radius and ranked:
            out['blast_radius'] = self._blast_radius()
        if self.level_shifts:
            shifted = self._rank_level_shifts(namespace)
            if shifted is not None:
                out['level_shift_root_causes'] = shifted
        if self.peer_deviations:
            peered = self._rank_peer_deviations(namespace)
            if peered is not None:
                out['peer_root_causes'] = peered
            if 'node_deviations' in results['metrics']:
                out['node_deviations'] = results['metrics']['node_deviations']
        if self.correlations:
            corr = self._correlations(namespace, ranked)
            if corr is not None:
                out['correlations'] = corr
        return out

    def _correlate_findings(self, *lists):  # ref :118-155
        """Group by component (first-seen order), keep groups with > 1 finding, max severity by
        SEVERITY_ORDER.  The group-by runs on the device (krca_group_reduce, f4): component ids
        interned here, severity index as the key; member lists are split on the host."""
        flat = [f for lst in lists for f in lst]
        if not flat:
            return []
        ids, comps = {}, []
        slot = np.empty(len(flat), np.int32)
        sev = np.empty(len(flat), np.int64)
        for i, f in enumerate(flat):
            c = f['component']
            slot[i] = j = ids.setdefault(c, len(ids))
            if j == len(comps):
                comps.append(c)
            s = f['severity']
            sev[i] = SEVERITY_ORDER.index(s) if type(s) is str and s in SEVERITY_ORDER else -1
        S = len(comps)
        first, count, n_key, top = self.engine.group_reduce(slot, sev, S, 1)
        order = np.argsort(slot, kind='stable')
        members = np.split(order, np.cumsum(count)[:-1])
        out = []
        for g in np.argsort(first, kind='stable').tolist():
            if count[g] < 2:
                continue
            if n_key[g] != count[g]:  # the reference's max(key=list.index) raises on the first bad one
                for i in members[g].tolist():
                    list(SEVERITY_ORDER).index(flat[i]['severity'])
            out.append({'component': comps[g], 'related_findings': [flat[i] for i in members[g].tolist()],
                        'correlation_type': 'component', 'severity': SEVERITY_ORDER[int(top[0, g])]})
        return out

    @staticmethod
    def _identify_root_causes(correlated):  # ref :157-184
        out = []
        for c in correlated:
            n = len(c['related_findings'])
            if c['severity'] in ('critical', 'high') and n > 1:
                out.append({'component': c['component'], 'related_findings_count': n, 'severity': c['severity'],
                            'explanation': f"High severity issue with {n} related findings indicates a potential root cause."})
        return out

    def _reset_agents(self):
        for a in (self.metrics_agent, self.logs_agent, self.traces_agent, self.topology_agent, self.events_agent):
            a.reset()

    # -- additive lead/lag correlations ------------------
    def _correlations(self, namespace, ranked):
        """lead_roots: anomalous pods that follow none of their dependencies and are followed by
        callers (ranked by those callers, then by anomaly); followers: per ranked root cause with a
        leading dependency, the strongest one, its lead in steps and r.  None without the bulk
        accessors (get_pod_metric_tensor and get_dependency_csr)."""
        from krca.leadlag import follower
        c = self.k8s_client
        scores = self.metrics_agent.last_scores
        if scores is None or not hasattr(c, 'get_pod_metric_tensor') or not hasattr(c, 'get_dependency_csr'):
            return None
        names, row_ptr, col, _ = c.get_dependency_csr(namespace)
        _, x = c.get_pod_metric_tensor(namespace)
        p = self.corr_params
        span = p['span'] if p['span'] is None else min(p['span'], int(x.shape[0]))
        edges = self.engine.corr_edges(x, row_ptr, col, channel=p['channel'], span=span, max_lag=p['max_lag'],
                                       tau=p['tau'], slack=p['slack'], host=False)
        index = {f"Pod/{n}": i for i, n in enumerate(names)}
        pods = [index[r['component']] for r in (ranked or []) if r['component'] in index]
        lr = self.engine.lead_roots(edges, scores['score'], k=min(int(self.rank_config.k), 16), explain=pods,
                                    row_ptr=row_ptr, col=col)
        roots = [{'component': f"Pod/{names[i]}", 'rank': r + 1, 'followers': int(f), 'anomaly': float(s)}
                 for r, (i, f, s) in enumerate(zip(lr['idx'].tolist(), lr['followers'].tolist(), lr['score'].tolist()))]
        foll = [follower(names[i], names[lr['explained'][i][0]], lr['explained'][i][1], lr['explained'][i][2])
                for i in pods if i in lr['explained']]
        return {'lead_roots': roots, 'followers': foll, 'params': dict(p)}

    # -- additive blast radius ----------------------------
    def _blast_radius(self):
        """Per ranked root cause: its transitive dependents, how many of them are anomalous and at
        which hop; the greedy cover of the anomalous nodes by the candidates' radii."""
        x = self._rank_ctx
        br = self.engine.blast_radius(x['row_ptr'], x['col'], x['idx'], pull=True, direction='dependents',
                                      bins=self.blast_bins, **x['mark'])
        return br.summary(names=[x['prefix'] + n for n in x['names']])

    # -- additive level-shift ranking ------------------------------------
    def _rank_level_shifts(self, namespace):
        """The rows of _rank_root_causes with the level-shift score as the seed ('anomaly' is that
        score); None without the bulk accessors or when the history is too short to score."""
        c = self.k8s_client
        sh = self.metrics_agent.last_shift
        if sh is None or not hasattr(c, 'get_dependency_csr'):
            return None
        names, row_ptr, col, outdeg = c.get_dependency_csr(namespace)
        idx, val, rank = self.engine.rank_root_causes(sh['score'], row_ptr, col, outdeg, self.rank_config,
                                                      n_metrics=int(sh['shift'].shape[1]))
        sc = sh['score_host']
        return [{'component': f"Pod/{names[i]}", 'rank': r + 1, 'score': float(v), 'pagerank': float(rank[i]),
                 'anomaly': float(sc[i])} for r, (i, v) in enumerate(zip(idx.tolist(), val.tolist()))]

    # -- additive peer-deviation ranking --------------------------------
    def _rank_peer_deviations(self, namespace):
        """The rows of _rank_root_causes with the peer deviation score as the seed ('anomaly' is that
        score); None without the bulk accessors or when nothing was scored."""
        c = self.k8s_client
        pr = self.metrics_agent.last_peer
        if pr is None or not hasattr(c, 'get_dependency_csr'):
            return None
        names, row_ptr, col, outdeg = c.get_dependency_csr(namespace)
        out = pr['service']
        idx, val, rank = self.engine.rank_root_causes(out['score'], row_ptr, col, outdeg, self.rank_config,
                                                      n_metrics=int(out['peer'].shape[1]))
        sc = out['score_host']
        return [{'component': f"Pod/{names[i]}", 'rank': r + 1, 'score': float(v), 'pagerank': float(rank[i]),
                 'anomaly': float(sc[i])} for r, (i, v) in enumerate(zip(idx.tolist(), val.tolist()))]

    # -- additive ranking ----------------------------------------------------------------
    def _rank_root_causes(self, namespace):
        c = self.k8s_client
        self._rank_ctx = None
        scores = self.metrics_agent.last_scores
        if scores is not None and hasattr(c, 'get_dependency_csr'):
            names, row_ptr, col, outdeg = c.get_dependency_csr(namespace)
            zl = scores.get('z_last')
            idx, val, rank = self.engine.rank_root_causes(scores['score'], row_ptr, col, outdeg, self.rank_config,
                                                          n_metrics=int(zl.shape[1]) if zl is not None else 1)
            sc = np.asarray(scores['score'].cpu() if hasattr(scores['score'], 'cpu') else scores['score'])
            self._rank_ctx = {'prefix': 'Pod/', 'names': names, 'row_ptr': row_ptr, 'col': col, 'idx': idx,
                              'mark': {'score': scores['score'], 'floor': self.rank_config.floor(
                                  len(outdeg), int(zl.shape[1]) if zl is not None else 1)}}
            return [{'component': f"Pod/{names[i]}", 'rank': r + 1, 'score': float(v), 'pagerank': float(rank[i]),
                     'anomaly': float(sc[i])} for r, (i, v) in enumerate(zip(idx.tolist(), val.tolist()))]
        if hasattr(c, 'get_service_dependencies') and hasattr(c, 'get_error_rate_by_service'):
            deps = c.get_service_dependencies()
            rates = c.get_error_rate_by_service()
            names = list(deps.keys())
            for ds in deps.values():
                for d in ds:
                    if d not in names:
                        names.append(d)
            pos = {n: i for i, n in enumerate(names)}
            src = [pos[s] for s, ds in deps.items() for _ in ds]
            dst = [pos[d] for _, ds in deps.items() for d in ds]
            row_ptr, col, outdeg = csr_from_edges(len(names), src, dst)
            seed = np.array([rates.get(n, 0.0) for n in names], dtype=np.float32)
            if not seed.sum() > 0:
                return None
            idx, val, rank = self.engine.rank_root_causes(seed, row_ptr, col, outdeg,
                                                          self.rank_config.replace(seed_floor=0.0))
            self._rank_ctx = {'prefix': 'Service/', 'names': names, 'row_ptr': row_ptr, 'col': col, 'idx': idx,
                              'mark': {'mark': seed > 0}}
            return [{'component': f"Service/{names[i]}", 'rank': r + 1, 'score': float(v), 'pagerank': float(rank[i]),
                     'anomaly': float(seed[i])} for r, (i, v) in enumerate(zip(idx.tolist(), val.tolist()))]
        return None
