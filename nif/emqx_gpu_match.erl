%% emqx_gpu_match — Erlang side of the GPU topic-matching NIF (spec + wrapper).
%% Built only where erl_nif.h / erlc exist (not in this container).
%%
%% Drop-in points (reference paths under apps/emqx/src):
%%   match_trie/1 in emqx_router.erl:137-141  -> match_batch/2
%%   match_routes/1 in emqx_router.erl:128-134 -> match_routes_batch/2 (+ lookup_routes/1 per filter)
%%   dispatch/2 in emqx_broker.erl:296-306    -> fanout_batch/2 (index from load_index/2)
%% The publish batching aggregator in front of these is
%% emqx_gpu_match_batcher (publish_batch/1).
%% On {error, _} the wrapper falls back to emqx_trie:match/1 (SURVEY.md §8b).
-module(emqx_gpu_match).

-export([load_index/1, load_index/2, load_index_sharded/1, load_index_sharded/2, update_index/2, update_subs/2,
         match_batch/2, match_routes_batch/2, fanout_batch/2, empty/1, export_index/1, import_index/1]).
-export([load_retained/1, load_retained/2, match_retained/3, expire_retained/2]).
-export([load_shared/3, load_shared/4, pick_shared/4, pick_shared_nif/5]).
-export([publish_window/4, publish_window_nif/5]).
-export([load_subopts/3, deliver/5, deliver_batches/5]).
-export([publish_window_deliver/7, publish_window_deliver_nif/9]).
-export([load_authz/1, authorize_batch/2, authz_rule/2, authz_request/3, authorize/5]).
-export([match/2]).

-on_load(init/0).

%% LoadInfo: the node's GPUs (application env `gpu_match_devices`, e.g.
%% [0,1,2,3,4,5,6,7]; a single ordinal is one GPU).  With a list, the one NIF
%% context replicates every index to all of them and spreads each batch over
%% them (emqx_gm_opts.n_devices).
%% `gpu_match_coalesce` (default false): LoadInfo becomes {coalesce, Devices}
%% and the NIF opens one emqx_gm_combiner on its context; match_batch/2,
%% match_routes_batch/2 and fanout_batch/2 then go through it, so the windows
%% of dirty schedulers that call at once -- every publisher matches in its own
%% process, emqx_broker.erl:204-215, emqx_trie.erl:66-70 -- share one device
%% round trip.  Results are the same either way.
init() ->
    Priv = case code:priv_dir(emqx) of {error, _} -> "priv"; D -> D end,
    Devices = application:get_env(emqx, gpu_match_devices, 0),
    Info = case application:get_env(emqx, gpu_match_coalesce, false) of
               true -> {coalesce, Devices};
               _ -> Devices
           end,
    erlang:load_nif(filename:join(Priv, "emqx_gpu_match_nif"), Info).

%% The route filters (emqx_route topics; wildcard ones are the emqx_trie
%% entries) -> an immutable index snapshot in HBM.
-spec load_index([binary()]) -> {ok, reference()} | {error, term()}.
load_index(_Filters) -> erlang:nif_error(nif_not_loaded).

%% Filters with their subscriber ids, one list per filter (the emqx_subscriber
%% bag, emqx_broker.erl:147-165, with its {shard, I} buckets flattened): the
%% index fanout_batch/2 needs.
-spec load_index([binary()], [[non_neg_integer()]]) -> {ok, reference()} | {error, term()}.
load_index(_Filters, _SubIds) -> erlang:nif_error(nif_not_loaded).

%% A route table too large for one GPU: the filters partitioned by first word
%% over the node's GPUs (the NIF context's device list), each topic matched on
%% its one GPU (emqx_gm_index_build_sharded).  Used like any index by the match
%% and fan-out calls.  update_index/2 works on a table loaded without subscriber
%% ids (load_index_sharded/1); with subscriber ids (load_index_sharded/2) it is
%% rebuild-only, and update_subs/2 and export_index/1 return {error, _} for any
%% sharded table.
-spec load_index_sharded([binary()]) -> {ok, reference()} | {error, term()}.
load_index_sharded(_Filters) -> erlang:nif_error(nif_not_loaded).

-spec load_index_sharded([binary()], [[non_neg_integer()]]) -> {ok, reference()} | {error, term()}.
load_index_sharded(_Filters, _SubIds) -> erlang:nif_error(nif_not_loaded).

%% Route changes (do_add_route/do_delete_route) as one batch -> a new snapshot;
%% the old one stays valid for readers holding it (emqx_gm_index_update).
%% Also on a table from load_index_sharded/1: each GPU applies its share.
%% Any op other than insert | delete is badarg.
-spec update_index(reference(), [{binary(), insert | delete}]) -> {ok, reference()} | {error, term()}.
update_index(_Index, _Ops) -> erlang:nif_error(nif_not_loaded).

%% emqx_gm_index_update_subs on an index from load_index/2: emqx_broker:subscribe/2
%% and unsubscribe/1 in one batch; a filter's first subscriber adds its route, the
%% last one leaving deletes it.  Any other op atom is badarg.
-spec update_subs(reference(), [{binary(), non_neg_integer(), subscribe | unsubscribe}]) ->
          {ok, reference()} | {error, term()}.
update_subs(_Index, _Ops) -> erlang:nif_error(nif_not_loaded).

-spec match_batch(reference(), [binary()]) -> [[binary()]] | {error, term()}.
match_batch(_Index, _Topics) -> erlang:nif_error(nif_not_loaded).

-spec match_routes_batch(reference(), [binary()]) -> [[binary()]] | {error, term()}.
match_routes_batch(_Index, _Topics) -> erlang:nif_error(nif_not_loaded).

%% Per topic: its matched filters, ascending, each with the subscriber ids
%% do_dispatch/2 folds over (a subscriber of two matching filters appears
%% under both: deliveries are a multiset).
-spec fanout_batch(reference(), [binary()]) -> [[{binary(), [non_neg_integer()]}]] | {error, term()}.
fanout_batch(_Index, _Topics) -> erlang:nif_error(nif_not_loaded).

-spec empty(reference()) -> boolean().
empty(_Index) -> erlang:nif_error(nif_not_loaded).

%% The snapshot as one binary (emqx_gm_index_export): what a node joining the
%% cluster imports instead of recompiling the route table -- the reference
%% replicates its routing tables through mria (emqx_router.erl:75-84).
-spec export_index(reference()) -> {ok, binary()} | {error, term()}.
export_index(_Index) -> erlang:nif_error(nif_not_loaded).

%% emqx_gm_index_import on this node's GPU; an image of another table layout
%% (another library build) is {error, _}.
-spec import_index(binary()) -> {ok, reference()} | {error, term()}.
import_index(_Image) -> erlang:nif_error(nif_not_loaded).

%% The retained-message table (emqx_retainer_mnesia.erl:74-104) as an index in
%% HBM: the subscribe direction.  Ids in match_retained/3 rows are positions in
%% Topics (of equal topics the last one); ExpiryMs 0 = never.  On a node with
%% several GPUs the table lives on the first one.
-spec load_retained([binary()]) -> {ok, reference()} | {error, term()}.
load_retained(_Topics) -> erlang:nif_error(nif_not_loaded).

-spec load_retained([binary()], [non_neg_integer()]) -> {ok, reference()} | {error, term()}.
load_retained(_Topics, _ExpiryMs) -> erlang:nif_error(nif_not_loaded).

%% emqx_retainer_mnesia:match_messages/1 (:210-214) per filter: the ids of the
%% stored topics it matches whose expiry is 0 or > NowMs, in topic order.  No
%% '$'-rule: <<"#">> returns <<"$SYS/...">> topics, as condition/1 does.
-spec match_retained(reference(), [binary()], non_neg_integer()) -> [[non_neg_integer()]] | {error, term()}.
match_retained(_Index, _Filters, _NowMs) -> erlang:nif_error(nif_not_loaded).

%% Set the expiry of stored topics in place: {Topic, 1} is delete_message/2 of
%% a literal topic (:117-128), {Topic, ExpiryMs} a refreshed message.  Returns
%% how many of the topics were stored.
-spec expire_retained(reference(), [{binary(), non_neg_integer()}]) -> {ok, non_neg_integer()} | {error, term()}.
expire_retained(_Index, _TopicExpiries) -> erlang:nif_error(nif_not_loaded).

%% The emqx_shared_subscription table (emqx_shared_sub.erl:287-288) bound to the
%% snapshot Index: one member list per {Filter, GroupId}, members in
%% subscription order; every Filter must be a filter of the snapshot (its shared
%% route).  Prev hands on the round_robin / sticky state of the slots both
%% tables hold (emqx_gm_shared_build).  On a node with several GPUs the table
%% lives on the first one.
-spec load_shared(reference(), [{binary(), non_neg_integer()}], [[non_neg_integer()]]) ->
          {ok, reference()} | {error, term()}.
load_shared(_Index, _Slots, _Members) -> erlang:nif_error(nif_not_loaded).

-spec load_shared(reference(), [{binary(), non_neg_integer()}], [[non_neg_integer()]], reference()) ->
          {ok, reference()} | {error, term()}.
load_shared(_Index, _Slots, _Members, _Prev) -> erlang:nif_error(nif_not_loaded).

%% emqx_shared_sub:dispatch/3's pick (pick/6, :234-288) for a whole publish
%% window: per message {Topic, ClientId}, in order, [{Filter, {GroupId,
%% MemberId}}] for every shared {Group, Filter} the topic matches.  The hash
%% strategies hash here, as do_pick_subscriber/6 does (:272-278); random draws
%% and unset round_robin / sticky starts derive from Seed.  FailedSubs and the
%% ack / nack retry of dispatch/4 (:118-130) stay with the caller.
-spec pick_shared(reference(), [{binary(), term()}], atom(), non_neg_integer()) ->
          [[{binary(), {non_neg_integer(), non_neg_integer()}}]] | {error, term()}.
pick_shared(Table, Msgs, Strategy, Seed) ->
    Topics = [T || {T, _} <- Msgs],
    {S, Hashes} = case Strategy of
                      hash_topic -> {0, [erlang:phash2(T) || {T, _} <- Msgs]};
                      H when H =:= hash; H =:= hash_clientid -> {0, [erlang:phash2(C) || {_, C} <- Msgs]};
                      round_robin -> {1, []};
                      sticky -> {2, []};
                      random -> {3, []}
                  end,
    pick_shared_nif(Table, Topics, S, Hashes, Seed band 16#FFFFFFFF).

%% Subscription options at dispatch (emqx_gm_subopts_build, emqx_gm_deliver).
%% load_subopts/3: the options of emqx_broker:subscribe/3 for the pairs of the
%% snapshot Index (from load_index/2): Opt = QoS bor (Nl bsl 2) bor (Rap bsl 3)
%% bor (UpgradeQoS bsl 4); a pair without an entry gets DefaultOpt
%% (?DEFAULT_SUBOPTS is 0).  The table is bound to Index and immutable.
-spec load_subopts(reference(), [{binary(), non_neg_integer(), 0..31}], 0..31) ->
          {ok, reference()} | {error, term()}.
load_subopts(_Index, _Entries, _DefaultOpt) -> erlang:nif_error(nif_not_loaded).

%% deliver/5: per topic, in order, {[{SubId, Byte}], Dropped}: the local
%% deliveries of fanout_batch/2 with the byte enrich_deliver/2 would compute
%% (QoS bor (Retain bsl 2) bor (NlFlag bsl 3)); Mode 0 marks a No-Local hit with
%% bit 4 (the session reproduces lists:dropwhile from it), Mode 1 removes it
%% and counts it in Dropped.  MsgFlags = PubQoS bor (Retain bsl 2) bor
%% (RetainedHeader bsl 3); From = the publisher's SubId or 16#FFFFFFFF.
-spec deliver(reference(), [binary()], [0..15], [non_neg_integer()], 0 | 1) ->
          [{[{non_neg_integer(), 0..31}], non_neg_integer()}] | {error, term()}.
deliver(_Table, _Topics, _MsgFlags, _From, _Mode) -> erlang:nif_error(nif_not_loaded).

%% deliver_batches/5: the same window by SUBSCRIBER (emqx_gm_deliver_batches):
%% [{SubId, [{Filter, {Row, Byte}}]}] by ascending SubId, each subscriber's
%% deliveries in window order -- the list its connection process would drain
%% from its mailbox (emqx_misc:drain_deliver/1) for emqx_channel:handle_deliver/2.
%% Row is the 0-based position of the message in Topics.  Mode 2 applies
%% emqx_session:ignore_local/4 itself: only the leading run of No-Local hits of a
%% list is removed (bit 4 cleared in what stays); a list it empties stays as
%% {SubId, []}.
-spec deliver_batches(reference(), [binary()], [0..15], [non_neg_integer()], 0 | 1 | 2) ->
          [{non_neg_integer(), [{binary(), {non_neg_integer(), 0..31}}]}] | {error, term()}.
deliver_batches(_Table, _Topics, _MsgFlags, _From, _Mode) -> erlang:nif_error(nif_not_loaded).

-spec pick_shared_nif(reference(), [binary()], 0..3, [non_neg_integer()], non_neg_integer()) ->
          [[{binary(), {non_neg_integer(), non_neg_integer()}}]] | {error, term()}.
pick_shared_nif(_Table, _Topics, _Strategy, _Hashes, _Seed) -> erlang:nif_error(nif_not_loaded).

%% A whole publish window in one device round trip (emqx_gm_publish_window): per
%% message {Topic, ClientId}, in order, {what fanout_batch/2 gives for the topic,
%% what pick_shared/4 gives for it} -- emqx_broker:publish/1's route + dispatch
%% and emqx_shared_sub:dispatch/3's pick, where the three calls would make five
%% waits on the device.  Table's snapshot must come from load_index/2.
-spec publish_window(reference(), [{binary(), term()}], atom(), non_neg_integer()) ->
          [{[{binary(), [non_neg_integer()]}], [{binary(), {non_neg_integer(), non_neg_integer()}}]}] |
          {error, term()}.
publish_window(Table, Msgs, Strategy, Seed) ->
    Topics = [T || {T, _} <- Msgs],
    {S, Hashes} = case Strategy of
                      hash_topic -> {0, [erlang:phash2(T) || {T, _} <- Msgs]};
                      H when H =:= hash; H =:= hash_clientid -> {0, [erlang:phash2(C) || {_, C} <- Msgs]};
                      round_robin -> {1, []};
                      sticky -> {2, []};
                      random -> {3, []}
                  end,
    publish_window_nif(Table, Topics, S, Hashes, Seed band 16#FFFFFFFF).

-spec publish_window_nif(reference(), [binary()], 0..3, [non_neg_integer()], non_neg_integer()) ->
          [{[{binary(), [non_neg_integer()]}], [{binary(), {non_neg_integer(), non_neg_integer()}}]}] |
          {error, term()}.
publish_window_nif(_Table, _Topics, _Strategy, _Hashes, _Seed) -> erlang:nif_error(nif_not_loaded).

%% A publish window whose local deliveries carry their option bytes
%% (emqx_gm_publish_window_deliver): per message {Topic, ClientId}, in order,
%% {what deliver/5 gives for the topic, what pick_shared/4 gives for it}, the
%% deliveries with their bytes computed in the window's one device round trip in
%% place of the plain fan-out.  Shared and SubOpts must be tables of the same
%% snapshot (load_index/2); MsgFlags, From and Mode as deliver/5 takes them.
-spec publish_window_deliver(reference(), reference(), [{binary(), term()}], atom(), non_neg_integer(),
                             {[0..15], [non_neg_integer()]}, 0 | 1) ->
          [{{[{non_neg_integer(), 0..31}], non_neg_integer()},
            [{binary(), {non_neg_integer(), non_neg_integer()}}]}] | {error, term()}.
publish_window_deliver(Shared, SubOpts, Msgs, Strategy, Seed, {MsgFlags, From}, Mode) ->
    Topics = [T || {T, _} <- Msgs],
    {S, Hashes} = case Strategy of
                      hash_topic -> {0, [erlang:phash2(T) || {T, _} <- Msgs]};
                      H when H =:= hash; H =:= hash_clientid -> {0, [erlang:phash2(C) || {_, C} <- Msgs]};
                      round_robin -> {1, []};
                      sticky -> {2, []};
                      random -> {3, []}
                  end,
    publish_window_deliver_nif(Shared, SubOpts, Topics, S, Hashes, Seed band 16#FFFFFFFF, MsgFlags, From, Mode).

-spec publish_window_deliver_nif(reference(), reference(), [binary()], 0..3, [non_neg_integer()], non_neg_integer(),
                                 [0..15], [non_neg_integer()], 0 | 1) ->
          [{{[{non_neg_integer(), 0..31}], non_neg_integer()},
            [{binary(), {non_neg_integer(), non_neg_integer()}}]}] | {error, term()}.
publish_window_deliver_nif(_Sh, _So, _Topics, _Strategy, _Hashes, _Seed, _Flags, _From, _Mode) -> erlang:nif_error(nif_not_loaded).

%% The authorization chain (file and built-in-database sources, in order) as
%% one table in HBM (emqx_gm_authz_build).  Segment = {Kind, [{Key, [Rule]}]}:
%% Kind 0 one rule list for every client ({<<>>, Rules}: a file source, or the
%% built-in database's `all` record), 1 / 2 the clientid / username records
%% (emqx_authz_mnesia.erl:123-132).  Rules come from authz_rule/2.  A table is
%% immutable: a changed ACL is a new load_authz/1 the caller swaps in.  On a node
%% with several GPUs the table lives on the first one.
-spec load_authz([{0..2, [{binary(), [tuple()]}]}]) -> {ok, reference()} | {error, term()}.
load_authz(_Segments) -> erlang:nif_error(nif_not_loaded).

%% emqx_authz:do_authorize/4 (emqx_authz.erl:307-317) for a window of requests
%% from authz_request/3, in order: {Verdict, RuleId} with Verdict 0 nomatch
%% (RuleId 16#FFFFFFFF), 1 allow, 2 deny.  No '$'-rule, as emqx_authz_rule has
%% none: <<"#">> authorizes <<"$SYS/x">>.
-spec authorize_batch(reference(), [tuple()]) -> [{0..2, non_neg_integer()}] | {error, term()}.
authorize_batch(_Table, _Requests) -> erlang:nif_error(nif_not_loaded).

%% A rule of the reference (emqx_authz_rule.erl:49, or {Permission, all}) with
%% the caller's id, in load_authz/1's form.  Regexes: the K-th distinct {re, _}
%% of the table (K < 32) is written {username | clientid, {re_bit, K}}; the
%% caller runs re:run/2 for each of them once per connection and hands the bits
%% to authz_request/3 as ReMask.
-spec authz_rule(non_neg_integer(), tuple()) -> tuple().
authz_rule(Id, {Permission, all}) ->
    authz_rule(Id, {Permission, all, all, [<<"#">>]});
authz_rule(Id, {Permission, Who, Action, Topics}) ->
    {Op, Leaves} = case Who of
                       all -> {0, []};
                       {'and', L} -> {0, L};
                       {'or', L} -> {1, L};
                       Leaf -> {0, [Leaf]}
                   end,
    {Id, perm_code(Permission), action_code(Action), Op,
     [authz_leaf(X) || X <- Leaves], [authz_filter(T) || T <- Topics]}.

perm_code(allow) -> 1;
perm_code(deny) -> 2.

action_code(publish) -> 1;
action_code(subscribe) -> 2;
action_code(all) -> 3.

authz_leaf({user, U}) -> authz_leaf({username, U});
authz_leaf({client, C}) -> authz_leaf({clientid, C});
authz_leaf({_, {re_bit, K}}) -> {3, <<K>>};
authz_leaf({username, U}) -> {0, iolist_to_binary(U)};
authz_leaf({clientid, C}) -> {1, iolist_to_binary(C)};
authz_leaf({ipaddr, CIDR}) -> {2, cidr_bytes(CIDR)};
authz_leaf({ipaddrs, CIDRs}) -> {2, iolist_to_binary([cidr_bytes(C) || C <- CIDRs])};
authz_leaf({'and', _}) -> {4, <<>>};   %% nested: refused by the library, as the reference's who() type has none
authz_leaf({'or', _}) -> {5, <<>>}.

%% esockd_cidr:parse(CIDR, true): family, lo, hi
cidr_bytes(CIDR) ->
    {Lo, Hi, _Len} = esockd_cidr:parse(CIDR, true),
    Fam = case tuple_size(Lo) of 4 -> 4; 8 -> 6 end,
    <<Fam, (addr_bytes(Lo))/binary, (addr_bytes(Hi))/binary>>.

addr_bytes({A, B, C, D}) -> <<A, B, C, D, 0:96>>;
addr_bytes(V6) -> << <<W:16>> || W <- tuple_to_list(V6) >>.

authz_filter({eq, T}) -> {1, iolist_to_binary(T)};
authz_filter(T) ->
    case iolist_to_binary(T) of
        <<"eq ", Rest/binary>> -> {1, Rest};
        Bin -> {0, Bin}
    end.

%% One request of authorize_batch/2 from the channel's clientinfo.
-spec authz_request(map(), publish | subscribe, binary()) -> tuple().
authz_request(ClientInfo, PubSub, Topic) ->
    Peer = case maps:get(peerhost, ClientInfo, undefined) of
               undefined -> undefined;
               {A, B, C, D} -> <<A, B, C, D>>;
               V6 -> addr_bytes(V6)
           end,
    {Topic, maps:get(clientid, ClientInfo, undefined), maps:get(username, ClientInfo, undefined), Peer,
     action_code(PubSub), maps:get(authz_re_mask, ClientInfo, 0)}.

%% The 'client.authorize' hook's callback with fallback: the verdict of the first
%% matching rule, DefaultResult on nomatch (authorization.no_match,
%% emqx_authz.erl:297-304), emqx_authz:authorize/5 on {error, _}.
-spec authorize(reference(), map(), publish | subscribe, binary(), allow | deny) -> {stop, allow | deny}.
authorize(Table, ClientInfo, PubSub, Topic, DefaultResult) ->
    case authorize_batch(Table, [authz_request(ClientInfo, PubSub, Topic)]) of
        [{1, _}] -> {stop, allow};
        [{2, _}] -> {stop, deny};
        [{0, _}] -> {stop, DefaultResult};
        {error, _} -> emqx_authz:authorize(ClientInfo, PubSub, Topic, DefaultResult, emqx_authz:lookup())
    end.

%% emqx_trie:match/1 drop-in with fallback.
-spec match(reference(), binary()) -> [binary()].
match(Index, Topic) when is_binary(Topic) ->
    case match_batch(Index, [Topic]) of
        [Row] -> Row;
        {error, _} -> emqx_trie:match(Topic)
    end.
