'use strict'
// What a Map / Array / Text document is, through the extension: node test/tojson.js --cpu|--gpu
//  --cpu : GpuMerge over an engine double built from the bundled yjs; checks what the extension asks of the engine
//          (one toJsonMany call per sharedJsonOf; versionSharedJson = restoreVersions, then one toJsonMany over the
//          fulfilled results)
//  --gpu : the same through the N-API addon (compat135: the bundle is yjs 13.5.16), string for string against yjs,
//          and the addon against the edge sessions of the committed fixture (tests/golden/tojson_v135.json.gz)
// A live board document (a Y.Map root holding cards: nested maps, a nested array, a nested text, a timestamp) and a
// document whose map holds a Uint8Array: sharedJsonOf equals JSON.stringify(getMap(root).toJSON()) on the live document;
// versionSharedJson on a restored version equals it on Y.createDocFromSnapshot; the binary document is left out and
// named.
const fs = require('fs')
const path = require('path')
const zlib = require('zlib')
const assert = require('assert')
const { GpuMerge, DocumentStore } = require('../src/index.js')

const mode = process.argv.includes('--gpu') ? 'gpu' : 'cpu'
const ROOT = path.join(__dirname, '..', '..', '..')
const Y = require(path.join(ROOT, 'tools', 'yjs_bundle.js')).load()   // the test oracle: yjs from the image's bundle
const { ask } = require(path.join(ROOT, 'tools', 'tojson_corpus.js'))   // the committed expectation over yjs's own document
const CODES = { 1: 'EMALFORMED', 3: 'ENONCANON', 9: 'EUNSUPPORTED' }

const load = (state, gc) => { const d = new Y.Doc({ gc }); Y.applyUpdate(d, state); return d }
const isNoGc = o => o === 1 || o === true || !!(o && o.gc === false)
const yjsRestore = (state, version, gc) => Y.encodeStateAsUpdate(Y.createDocFromSnapshot(load(state, false), Y.decodeSnapshot(version), new Y.Doc({ gc })))
const restoreOr = (s, v, gc) => { try { return yjsRestore(s, v, gc) } catch (e) { return Object.assign(new Error(String(e.message)), { code: 'EINVAL' }) } }
const toJsonOr = (state, name, kind) => { const r = ask(state, name, kind); return r[2] === 0 ? r[3] : Object.assign(new Error('refused'), { code: CODES[r[2]] }) }

// test double (never shipped): the engine calls the extension makes, from yjs
class Double {
  constructor () { this.log = [] }
  async mergeUpdates (updates) { return Y.mergeUpdates(updates) }
  async mergeMany (docs) { return docs.map(u => Y.mergeUpdates(u)) }
  async snapshot (update, opts) { return Y.encodeStateAsUpdate(load(update, !(opts && opts.gc === false))) }
  async takeVersionMany (states) { return states.map(s => Y.encodeSnapshot(Y.snapshot(load(s, true)))) }
  async restoreVersionMany (states, versions, opts) { return states.map((s, i) => restoreOr(s, versions[i], !(opts && isNoGc(opts[i])))) }
  async toJsonMany (states, names, kind) {
    this.log.push(['toJsonMany', states.length, Array.from(names), kind])
    return states.map((s, i) => toJsonOr(s, String(names[i]), kind))
  }
  close () {}
}

class MemoryStore extends DocumentStore {
  constructor () { super(); this.rows = new Map() }
  async fetchMany (payloads) { return payloads.map(p => this.rows.get(p.documentName) || null) }
  async storeMany (entries) { for (const e of entries) this.rows.set(e.payload.documentName, Uint8Array.from(e.state)) }
}

async function openDoc (ext, name, gc, id) {
  const document = new Y.Doc({ gc })
  document.clientID = id
  document.name = name
  const payload = { document, documentName: name, context: {}, requestParameters: new Map() }
  await ext.onLoadDocument(payload)
  await ext.afterLoadDocument(payload)
  return payload
}

function makeEngine () {
  if (mode === 'cpu') return new Double()
  const { GpuEngine } = require('../src/engine.js')
  return new GpuEngine({ device: 0, batchWindowMs: 5, compat135: true })
}

function card (cards, id, title) {
  const c = new Y.Map()
  cards.set(id, c)
  c.set('title', title); c.set('done', false); c.set('updatedAt', 1700000000000 + cards.size)
  const tags = new Y.Array(); c.set('tags', tags); tags.push(['new', { color: 'red' }])
  const body = new Y.Text(); c.set('body', body); body.insert(0, 'Body of "' + title + '" 😀')
  return c
}

test_('sharedJsonOf and versionSharedJson of a board document; a document holding binary content is left out and named', async () => {
  const engine = makeEngine()
  const ext = new GpuMerge({ engine, store: new MemoryStore(), Y })
  try {
    const x = await openDoc(ext, 'board', false, 41)
    const b = await openDoc(ext, 'binary', false, 42)
    const cards = x.document.getMap('cards')
    const now = (doc, root, kind) => JSON.stringify((kind === 1 ? load(Y.encodeStateAsUpdate(doc), true).getArray(root) : load(Y.encodeStateAsUpdate(doc), true).getMap(root)).toJSON())
    const c1 = card(cards, 'c1', 'First')
    card(cards, '7', 'Seven')
    x.document.getArray('order').push(['c1', '7'])
    b.document.getMap('cards').set('blob', new Uint8Array([1, 2, 3]))
    const v0 = (await ext.takeVersions(['board'])).get('board')
    const at0 = now(x.document, 'cards', 0)
    c1.set('done', true); c1.get('tags').delete(0, 1); c1.get('body').delete(0, 5); cards.delete('7'); card(cards, 'c3', 'Third')

    const got = await ext.sharedJsonOf(['board', 'missing', 'binary'], { root: 'cards' })
    assert.deepStrictEqual(Array.from(got.keys()), ['board'])
    assert.strictEqual(got.get('board'), now(x.document, 'cards', 0))
    assert.deepStrictEqual(ext.unserialized, [{ documentName: 'binary', code: 'EUNSUPPORTED' }])
    const obj = (await ext.sharedJsonOf(['board'], { root: 'cards', parse: true })).get('board')
    assert.deepStrictEqual(Object.keys(obj), ['c1', 'c3'])
    assert.deepStrictEqual(obj.c1, { title: 'First', done: true, updatedAt: 1700000000001, tags: [{ color: 'red' }], body: 'of "First" 😀' })
    assert.strictEqual((await ext.sharedJsonOf(['board'], { root: 'order', type: 'array' })).get('board'), '["c1","7"]')
    assert.strictEqual((await ext.sharedJsonOf(['board'], { root: 'other', type: 'text' })).get('board'), '""')
    assert.strictEqual((await ext.sharedJsonOf(['board'])).get('board'), '{}')
    await assert.rejects(ext.sharedJsonOf(['board'], { type: 'xml' }), TypeError)
    if (mode === 'cpu') {
      assert.deepStrictEqual(engine.log, [['toJsonMany', 2, ['cards', 'cards'], 0], ['toJsonMany', 1, ['cards'], 0], ['toJsonMany', 1, ['order'], 1],
        ['toJsonMany', 1, ['other'], 2], ['toJsonMany', 1, ['default'], 0]])
      engine.log.length = 0
    }

    // versionSharedJson: toJSON on Y.createDocFromSnapshot; an unknown document rejects alone
    const res = await ext.versionSharedJson([{ documentName: 'board', version: v0 }, { documentName: 'gone', version: v0 }], { root: 'cards' })
    assert.deepStrictEqual(res.map(r => r.status), ['fulfilled', 'rejected'])
    assert.strictEqual(res[0].value, now(Y.createDocFromSnapshot(x.document, Y.decodeSnapshot(v0)), 'cards', 0))
    assert.strictEqual(res[0].value, at0)
    assert.deepStrictEqual(Object.keys(JSON.parse(res[0].value)), ['7', 'c1'])   // (an index key comes first)
    const parsed = await ext.versionSharedJson([{ documentName: 'board', version: v0 }], { root: 'cards', parse: true })
    assert.deepStrictEqual(parsed[0].value, JSON.parse(at0))
    if (mode === 'cpu') assert.deepStrictEqual(engine.log, [['toJsonMany', 1, ['cards'], 0], ['toJsonMany', 1, ['cards'], 0]])
  } finally { engine.close() }
})

if (mode === 'gpu') {
  test_('the addon against the fixture\'s edge sessions, and the pool: strings in caller order, refusals alone', async () => {
    const { GpuEngine, GpuEnginePool, TOJSON_MAP, TOJSON_ARRAY, TOJSON_TEXT } = require('../src/engine.js')
    assert.deepStrictEqual([TOJSON_MAP, TOJSON_ARRAY, TOJSON_TEXT], [0, 1, 2])
    const engine = new GpuEngine({ device: 0, compat135: true })
    try {
      const fix = JSON.parse(zlib.gunzipSync(fs.readFileSync(path.join(ROOT, 'tests', 'golden', 'tojson_v135.json.gz'))).toString())
      let n = 0
      for (const kind of [0, 1, 2]) {
        const rows = []
        for (const e of fix.edges) for (const r of e.asks) if (r[1] === kind) rows.push([e.note, Buffer.from(e.state, 'hex'), Buffer.from(r[0], 'hex'), r[2], Buffer.from(r[3], 'hex').toString('utf8')])
        const got = await engine.toJsonMany(rows.map(r => r[1]), rows.map(r => r[2]), kind)
        rows.forEach((r, i) => {
          if (r[3] === 0) assert.strictEqual(got[i], r[4], r[0])
          else assert.ok(got[i] instanceof Error && got[i].code === CODES[r[3]], r[0] + ': ' + String(got[i]))
        })
        n += rows.length
      }
      assert.ok(n >= 45, String(n))
      assert.deepStrictEqual(await engine.toJsonMany([], [], 0), [])
      const u = Buffer.from(fix.edges[2].state, 'hex')
      await assert.rejects(engine.toJsonMany([u], [], 0), x => x.code === 'EINVAL')
      await assert.rejects(engine.toJsonMany([u], ['m'], 3), x => x.code === 'EINVAL')
      const pool = new GpuEnginePool({ makeEngine: () => engine, devices: [0] })
      assert.deepStrictEqual(await pool.toJsonMany(['a', 'b'], [u, u], ['m', 'absent'], 0), ['{"9":"v9","10":"v10","a":"va","04":"v04"}', '{}'])
    } finally { engine.close() }
  })
}

function test_ (name, fn) { (test_.all = test_.all || []).push({ name, fn }) }

;(async () => {
  let failed = 0
  for (const t of test_.all) {
    try { await t.fn(); console.log('ok   ' + t.name) } catch (e) { failed++; console.log('FAIL ' + t.name + '\n' + (e && e.stack || e)) }
  }
  console.log(failed ? failed + ' failed' : test_.all.length + ' passed (' + mode + ')')
  process.exit(failed ? 1 : 0)
})()
